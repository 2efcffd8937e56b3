"""A population of conv DQN agents trained in one launch chain: drl_convpop_*
(dronerl_amd/csrc/convpop/), dronerl_amd.population.ConvPopulationDQN,
train_population(network_type="conv") and `python -m dronerl_amd.conv_sweep`.

Reference: run_jax_sweep.py, which draws network_type from ['dense', 'conv'];
each member is train_jax.py:38-115's learner block with network_type 'conv'.

The yardsticks are code that exists without the population: the single-agent
LargeBatchConvDQNLearner (drl_convnet_dqn_large_train) for the learner, and
tests/_conv_pop_ref.py, a numpy restatement of cl_forward's summation order,
for the act.  Every GPU comparison is BIT FOR BIT: no tolerance anywhere.
"""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _conv_learner_ref as R
from tests import _conv_pop_ref as F32
from oracle import dqn_learner as O
from test_dqn import _hash_explore

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SETS = ("online", "target", "m", "v")
vp = ctypes.c_void_p
NETS = {k: R.NETS[k] for k in ("b", "c", "g", "i")}
# the env of each net: its window's radius (b, i: W 7; c: W 9; g: W 5)
SHAPES = {"b": dict(n_drones=4, grid_size=9, window_radius=3), "i": dict(n_drones=8, grid_size=16, window_radius=3),
          "g": dict(n_drones=8, grid_size=16, window_radius=2), "c": dict(n_drones=8, grid_size=16, window_radius=4)}


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind, _bind_convnet
    from dronerl_amd.population import _bind_convpop, _bind_pop
    return _bind_convpop(_bind_pop(_bind(_bind_convnet(lib()))))


def _desc(name="b", inp="code", n_actions=5):
    from dronerl_amd.dqn import convnet_desc
    W, conv, dense = R.NETS[name]
    return convnet_desc((W, W, 6), conv, dense, n_actions, inp)


# ------------------------------------------------------------------- CPU ---
def test_convpop_layout_places_every_word_once(tmp_path):
    """tests/native/convpop_layout_check.cpp, a stand-alone program under the
    address and undefined-behaviour sanitizers (nothing is loaded into
    Python): for three nets x members {1, 3} x max_batch {1, 64, 65, 130}
    member blocks do not overlap, each equals cg::plan's block at max_batch,
    the records are 16-byte aligned behind the last block, every word of the
    layout is placed once."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "convpop_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "convpop_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_convpop_member_block_is_the_single_agents():
    """drl_convpop_layout_query's member block equals
    drl_convnet_dqn_large_layout_query's at max_batch, field by field."""
    from dronerl_amd.dqn import DrlConvnetDqnLayout
    from dronerl_amd.population import DrlConvPopLayout
    L = _lib()

    def _fields(lay_):
        return {f: (list(getattr(lay_, f)) if hasattr(getattr(lay_, f), "__len__") else getattr(lay_, f))
                for f, _ in DrlConvnetDqnLayout._fields_}
    for name, batch, P in (("b", 8, 1), ("c", 65, 3), ("g", 130, 5), ("i", 4096, 1024)):
        lay, one, d = DrlConvPopLayout(), DrlConvnetDqnLayout(), _desc(name)
        assert L.drl_convpop_layout_query(ctypes.byref(d), P, batch, ctypes.byref(lay)) == 0, L.drl_last_error()
        assert L.drl_convnet_dqn_large_layout_query(ctypes.byref(d), batch, ctypes.byref(one)) == 0
        assert _fields(lay.member) == _fields(one)
        assert lay.member_stride % 16 == 0 and lay.member_stride >= lay.member.bytes
        assert lay.hparams_off == lay.member_stride * P and lay.hparams_off % 16 == 0
        assert lay.hparams_stride == 96 and lay.bytes >= lay.hparams_off + P * lay.hparams_stride
        assert (lay.members, lay.max_batch) == (P, batch)


def test_convpop_calls_validate_before_device_work():
    """Every call is refused before any device work (no GPU), with its
    reason: input != code, window 3, members 0 and 1025, max_batch 0 and
    4097, a member batch above max_batch, a NULL block, and the other NULL
    pointers and empty calls."""
    from dronerl_amd.dqn import DQNHParams, DrlDqnHParams, DrlReplay, convnet_desc
    from dronerl_amd.population import DrlConvPopLayout
    L = _lib()
    E = L.drl_last_error
    good, lay = _desc("b"), DrlConvPopLayout()
    ring = DrlReplay(50, 32, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    blk, ptr = vp(1 << 20), vp(1 << 21)
    hp4 = (DrlDqnHParams * 4)(*[DQNHParams(batch=8).c() for _ in range(4)])
    eps4 = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)

    def every_call(d, P, B):
        """Each call with the same (description, members, max_batch): all must refuse."""
        return [
            L.drl_convpop_layout_query(d, P, B, ctypes.byref(lay)),
            L.drl_convpop_init(d, P, B, hp4, eps4, blk, None),
            L.drl_convpop_act(d, P, B, blk, ptr, 4, 0, 0, 0, 0, ptr, 4, 0, 0, None, None),
            L.drl_convpop_train(d, P, B, blk, ctypes.byref(ring), 10, None),
            L.drl_convpop_sample_rows(d, P, B, blk, 10, ptr, None),
        ]

    w3 = convnet_desc((3, 3, 6), (R._c(8, 1, 1, 0),), (8,), 5, "code")
    k6 = _desc("b")
    k6.conv[0].kernel_size = 6
    for d, P, B, word in ((good, 0, 8, b"members"), (good, 1025, 8, b"members"), (good, -1, 8, b"members"),
                          (good, 4, 0, b"max_batch"), (good, 4, 4097, b"max_batch"),
                          (_desc("b", "obs"), 4, 8, b"policy code"), (w3, 4, 8, b"window"),
                          (k6, 4, 8, b"kernel_size"), (_desc("b", n_actions=9), 4, 8, b"n_actions"),
                          (None, 4, 8, b"NULL")):
        dd = None if d is None else ctypes.byref(d)
        for rc in every_call(dd, P, B):
            assert rc != 0 and word in E(), (word, E())
    d = ctypes.byref(good)
    assert L.drl_convpop_layout_query(d, 4, 8, None) != 0 and b"layout is NULL" in E()
    # init: the member's batch, the schedule, the pointers
    bad = (DrlDqnHParams * 4)(*[DQNHParams(batch=b).c() for b in (8, 8, 9, 8)])
    assert L.drl_convpop_init(d, 4, 8, bad, eps4, blk, None) != 0 and b"member 2: batch must be in [1, max_batch]" in E()
    bad = (DrlDqnHParams * 4)(*[DQNHParams(batch=b).c() for b in (8, 0, 8, 8)])
    assert L.drl_convpop_init(d, 4, 8, bad, eps4, blk, None) != 0 and b"member 1: batch" in E()
    bad = (DrlDqnHParams * 4)(*[DQNHParams(batch=8, target_update_interval=t).c() for t in (1, 1, 1, 0)])
    assert L.drl_convpop_init(d, 4, 8, bad, eps4, blk, None) != 0 and b"member 3: target_update_interval" in E()
    bad = (DrlDqnHParams * 4)(*[DQNHParams(batch=8, beta2=b).c() for b in (1.0, 0.9, 0.9, 0.9)])
    assert L.drl_convpop_init(d, 4, 8, bad, eps4, blk, None) != 0 and b"member 0: beta1" in E()
    assert L.drl_convpop_init(d, 4, 8, None, eps4, blk, None) != 0 and b"hparams is NULL" in E()
    assert L.drl_convpop_init(d, 4, 8, hp4, None, blk, None) != 0 and b"epsilon_start is NULL" in E()
    assert L.drl_convpop_init(d, 4, 8, hp4, eps4, None, None) != 0 and b"population block" in E()
    assert L.drl_convpop_init(d, 4, 8, hp4, eps4, vp((1 << 20) + 8), None) != 0 and b"16-byte" in E()
    # act
    act = lambda pop=blk, code=ptr, E_=4, acts=ptr, N=4, q=None: L.drl_convpop_act(  # noqa: E731
        d, 4, 8, pop, code, E_, 0, 0, 0, 0, acts, N, 0, 0, q, None)
    assert act(pop=None) != 0 and b"population block" in E()
    assert act(code=None) != 0 and b"policy code" in E()
    assert act(code=vp((1 << 21) + 8)) != 0 and b"16-byte" in E()
    assert act(E_=0) != 0 and b"envs_per_member" in E()
    assert act(acts=None) != 0 and b"actions" in E()
    assert act(q=vp((1 << 21) + 2)) != 0 and b"4-byte" in E()
    assert act(N=0) != 0 and b"n_drones" in E()
    assert act(N=65) != 0 and b"n_drones" in E()
    # train
    train = lambda pop=blk, r=ring, size=10: L.drl_convpop_train(  # noqa: E731
        d, 4, 8, pop, None if r is None else ctypes.byref(r), size, None)
    assert train(pop=None) != 0 and b"population block" in E()
    assert train(r=None) != 0 and b"replay" in E()
    assert train(r=DrlReplay(50, 32, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"NULL" in E()
    assert train(r=DrlReplay(0, 32, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"capacity" in E()
    assert train(size=-1) != 0 and b"size" in E()
    assert train(size=51) != 0 and b"size" in E()
    assert train(r=DrlReplay(50, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"policy codes" in E()
    # sample rows
    assert L.drl_convpop_sample_rows(d, 4, 8, None, 10, ptr, None) != 0 and b"population block" in E()
    assert L.drl_convpop_sample_rows(d, 4, 8, blk, 10, None, None) != 0 and b"d_slots" in E()
    assert L.drl_convpop_sample_rows(d, 4, 8, blk, 10, vp((1 << 21) + 4), None) != 0 and b"d_slots" in E()
    assert L.drl_convpop_sample_rows(d, 4, 8, blk, 0, ptr, None) != 0 and b"size" in E()


def test_conv_sweep_cli_grid_seeds_and_refusals():
    """conv_sweep.parse_args: the grid and the seeds through sweep's shared
    functions, the conv options, the refusal of --use_sharding and of dense;
    dronerl_amd.sweep keeps refusing conv."""
    from dronerl_amd import conv_sweep, sweep
    assert conv_sweep.expand_grid is sweep.expand_grid and conv_sweep.members_of is sweep.members_of
    args, points = conv_sweep.parse_args([
        "--grid", '{"learning_rate": [1e-4, 5e-4], "batch_size": [8, 16]}', "--members_seeds", "3", "--num_envs", "4",
        "--num_steps", "40", "--seed", "5", "--gamma", "0.8", "--conv_layers",
        '[{"out_channels": 16, "kernel_size": 3, "padding": 1}, {"out_channels": 32, "kernel_size": 3, "padding": 1}]',
        "--conv_dense_layers", "128", "64"])
    assert args.network_type == "conv" and (args.num_envs, args.num_steps, args.members_seeds) == (4, 40, 3)
    assert [c["out_channels"] for c in args.conv_layers] == [16, 32] and tuple(args.conv_dense_layers) == (128, 64)
    assert points == sweep.expand_grid({"learning_rate": [1e-4, 5e-4], "batch_size": [8, 16]})
    hps, seeds, rows = conv_sweep.members_of(args, points)
    assert len(hps) == 12 and seeds == [5, 6, 7] * 4
    assert [hp.batch for hp in hps] == [8] * 3 + [16] * 3 + [8] * 3 + [16] * 3
    assert [hp.learning_rate for hp in hps] == [1e-4] * 6 + [5e-4] * 6
    assert all(hp.gamma == 0.8 and hp.num_steps == 40 for hp in hps) and [hp.sample_seed for hp in hps] == seeds
    assert rows[4] == {"learning_rate": 1e-4, "batch_size": 16, "seed": 6}
    a2, p2 = conv_sweep.parse_args([])
    assert p2 == [{}] and a2.members_seeds == 1 and a2.network_type == "conv"
    assert len(a2.conv_layers) == 1 and a2.conv_layers[0]["out_channels"] == 8  # train_jax's default conv net
    a3, _ = conv_sweep.parse_args(["--network_type", "conv"])
    assert a3.network_type == "conv"
    with pytest.raises(ValueError, match="dronerl_amd.sweep"):
        conv_sweep.parse_args(["--network_type", "dense"])
    with pytest.raises(ValueError, match="use_sharding"):
        conv_sweep.parse_args(["--use_sharding", "--num_envs", "4"])
    with pytest.raises(ValueError, match="hidden_layers must be shared"):
        conv_sweep.parse_args(["--grid", '{"hidden_layers": [[16], [32]]}'])
    with pytest.raises(ValueError, match="not valid JSON"):
        conv_sweep.parse_args(["--grid", "{learning_rate: 1}"])
    with pytest.raises(ValueError, match="members_seeds"):
        conv_sweep.parse_args(["--members_seeds", "0"])
    with pytest.raises(ValueError, match="at most 1024"):
        conv_sweep.parse_args(["--grid", json.dumps({"gamma": [0.9] * 33, "tau": [1.0] * 32})])
    with pytest.raises(ValueError, match="dense nets only"):
        sweep.parse_args(["--network_type", "conv"])


def test_train_population_refuses_an_unknown_network_type():
    from dronerl_amd import EnvParams
    from dronerl_amd.population import train_population
    with pytest.raises(ValueError, match="network_type"):
        train_population(EnvParams(), [], 1, 1, network_type="resnet")


@pytest.mark.parametrize("name", sorted(NETS))
def test_f32_restatement_is_the_conv_forward(name):
    """tests/_conv_pop_ref.forward (float32, cl_forward's order) against
    tests/_conv_learner_ref.forward in float64 on synthetic windows, within
    that file's own rule: max(1e-5, 4 x rel(torch-f32 forward, f64 forward))."""
    W, conv, dense = NETS[name]
    seed = 40 + ord(name)
    ps = R.random_params(W, conv, dense, seed)
    x = R.synthetic_windows(W, 24, seed + 1)
    flat = lambda dt: [torch.tensor(t, dtype=dt) for wb in ps for t in wb]  # noqa: E731
    q64 = R.forward(flat(torch.float64), conv, torch.tensor(x, dtype=torch.float64).reshape(-1, W, W, 6)).numpy()
    q32 = R.forward(flat(torch.float32), conv, torch.tensor(x).reshape(-1, W, W, 6)).numpy()
    mine = F32.forward(ps, conv, x, W)
    assert mine.dtype == np.float32 and mine.shape == q64.shape
    got, tol = R.rel(mine, q64), R.tolerance(q32, q64)
    print(f"net {name}: rel {got:.3g}, tolerance {tol:.3g}")
    assert got <= tol


# Every __global__ kernel under csrc/convpop/ and the -m gpu test that launches it.
_T = "test_conv_population.py::"
KERNEL_TESTS = {
    "drl_convpop_init_kernel": _T + "test_convpop_learner_equals_the_single_agent_bit_exact",
    "drl_convpop_act_kernel": _T + "test_convpop_act_is_the_learners_forward_bit_exact",
    "drl_convpop_rows_kernel": _T + "test_convpop_learner_equals_the_single_agent_bit_exact",
    "drl_convpop_dense_grad_kernel": _T + "test_convpop_learner_equals_the_single_agent_bit_exact",
    "drl_convpop_conv_grad_kernel": _T + "test_convpop_learner_equals_the_single_agent_bit_exact",
    "drl_convpop_update_kernel": _T + "test_convpop_learner_equals_the_single_agent_bit_exact",
    "drl_convpop_counters_kernel": _T + "test_convpop_learner_equals_the_single_agent_bit_exact",
    "drl_convpop_sample_kernel": _T + "test_convpop_sample_slots_are_each_members_draws",
}


def test_every_convpop_kernel_has_a_gpu_test():
    import glob
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "convpop", "*.hip")):
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
def _host(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rand_sets(name, P, seed):
    """Per member ([W], [b]) with random weights AND biases, online and target (tests/_conv_learner_ref.py)."""
    W, conv, dense = NETS[name]

    def one(s):
        ws, bs = zip(*R.random_params(W, conv, dense, s))
        return [torch.tensor(w) for w in ws], [torch.tensor(b) for b in bs]
    return [one(seed + 2 * m) for m in range(P)], [one(seed + 2 * m + 1) for m in range(P)]


def _setup(name, hps, E, cap, seed=0, env_offset=0, guard=0, online=None, target=None, max_batch=None):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.population import ConvPopulationDQN, PopulationReplay
    W, conv, dense = NETS[name]
    ep = EnvParams(**SHAPES[name])
    P = len(hps)
    env = BatchedDeliveryDrones(ep, P * E, env_offset=env_offset)
    env.reset(seed=seed)
    if online is None:
        online, target = _rand_sets(name, P, seed + 11)
    pop = ConvPopulationDQN((W, W, 6), conv, dense, hps, E, online=online, target=target, guard_bytes=guard,
                            max_batch=max_batch)
    rb = PopulationReplay(P, cap, ep.window_radius)
    return env, pop, rb


class _Loop:
    """train_population's loop shape, a step at a time: act -> step -> add (the caller trains)."""

    def __init__(self, env, pop, rb, act_seed=3, synth_seed=5):
        self.env, self.pop, self.rb, self.act_seed, self.synth_seed = env, pop, rb, act_seed, synth_seed
        self.cur, self.nxt = env.new_code(), env.new_code()
        env.get_code(out=self.cur)
        self.acts = torch.empty((env.num_envs, env.n_drones), dtype=torch.int32, device="cuda")
        self.t = 0

    def fill(self):
        self.pop.act(self.cur, self.t, seed=self.act_seed, env_offset=self.env.env_offset, actions=self.acts,
                     synth=(self.synth_seed, self.t))
        self.rew, self.don = self.env.step(self.acts, code=self.nxt)
        self.rb.add(self.cur, self.acts, self.rew, self.nxt, self.don)
        self.cur, self.nxt = self.nxt, self.cur
        self.t += 1


@gpu
@pytest.mark.parametrize("E", [1, 3, 17])
@pytest.mark.parametrize("name", ["b", "c", "g", "i"])
def test_convpop_act_is_the_learners_forward_bit_exact(name, E):
    """P = 3 members with different random parameters at epsilon 0.0, 0.5 and
    1.0, codes from a reset env a few steps in: Q of every env equals the
    numpy restatement of cl_forward (inputs from dqn.decode_policy_code) bit
    for bit; column 0 is the explore draw at the member's device epsilon or
    the first argmax of that Q -- for every env, since Q is bit-equal --;
    columns 1.. equal synth_actions; the sentinels behind the action and Q
    buffers are intact; the greedy flag ignores epsilon."""
    from dronerl_amd.dqn import DQNHParams, decode_policy_code
    W, conv, dense = NETS[name]
    P, A = 3, 5
    eps = [0.0, 0.5, 1.0]
    hps = [DQNHParams(batch=8, epsilon_start=e, epsilon_decay=1.0, epsilon_end=0.0) for e in eps]
    env, pop, _ = _setup(name, hps, E, 16, seed=2, env_offset=1000)
    N, n = env.n_drones, P * E
    for t in range(3):  # (a few random steps: drones in the windows, charges below 100)
        env.step(env.synth_actions(9, t))
    code = env.get_code()
    SENT = 0x5A5A5A5A
    abuf = torch.full((n * N + 64,), SENT, dtype=torch.int32, device="cuda")
    qbuf = torch.full((n * A + 64,), float("nan"), dtype=torch.float32, device="cuda")
    acts, q = abuf[:n * N].view(n, N), qbuf[:n * A].view(n, A)
    pop.act(code, 6, seed=3, env_offset=env.env_offset, actions=acts, synth=(5, 6), q_out=q)
    X = _host(decode_policy_code(code, env.params.window_radius)).reshape(n, -1)[:, :W * W * 6]
    a_h, q_h = _host(acts), _host(q)
    wants = []
    for m in range(P):
        s = slice(m * E, (m + 1) * E)
        ps = [(_host(w), _host(b)) for w, b in pop.params("online", m)]
        want = F32.forward(ps, conv, X[s], W)
        wants.append(want)
        assert np.array_equal(_bits(q_h[s]), _bits(want)), ("Q", m, np.abs(q_h[s] - want).max())
        explored = 0
        for e in range(E):
            explore, rnd = _hash_explore(3, 6, 1000 + m * E + e, A, eps[m])
            explored += int(explore)
            assert a_h[m * E + e, 0] == (rnd if explore else int(np.argmax(want[e]))), (m, e)
        assert explored == (0 if eps[m] == 0.0 else E if eps[m] == 1.0 else explored)
    assert np.array_equal(a_h[:, 1:], _host(env.synth_actions(5, 6))[:, 1:])
    assert bool((abuf[n * N:] == SENT).all()) and bool(torch.isnan(qbuf[n * A:]).all())
    # greedy: the argmax everywhere, whatever epsilon holds; no Q buffer
    abuf.fill_(SENT)
    pop.act(code, 6, seed=3, env_offset=env.env_offset, actions=acts, synth=(5, 6), greedy=True)
    g_h = _host(acts)
    for m in range(P):
        assert np.array_equal(g_h[m * E:(m + 1) * E, 0], np.argmax(wants[m], axis=1).astype(np.int32)), ("greedy", m)
    assert np.array_equal(g_h[:, 1:], a_h[:, 1:]) and bool((abuf[n * N:] == SENT).all())


def _learner_hps():
    from dronerl_amd.dqn import DQNHParams
    kw = dict(epsilon_decay_every=1)
    return [DQNHParams(batch=1, gamma=0.9, learning_rate=1e-3, sample_seed=1, epsilon_decay=0.9, **kw),
            DQNHParams(batch=8, gamma=0.95, learning_rate=3e-3, tau=0.6, target_update_interval=3, sample_seed=2,
                       epsilon_decay=0.8, **kw),
            DQNHParams(batch=64, gamma=0.8, learning_rate=5e-4, target_update_interval=2, sample_seed=3,
                       epsilon_decay=0.95, epsilon_end=0.2, **kw),
            DQNHParams(batch=65, gamma=0.99, learning_rate=2e-3, tau=0.6, target_update_interval=3, sample_seed=4,
                       epsilon_decay=0.7, **kw),
            DQNHParams(batch=130, gamma=0.85, learning_rate=7e-4, tau=0.6, target_update_interval=3, sample_seed=5,
                       epsilon_decay=0.85, **kw)]


def _single_agents(name, hps, online, target, cap, radius):
    """Per member a LargeBatchConvDQNLearner (the single-agent chain) with the member's net, initial sets and
    hyperparameters, and a ReplayBuffer to hold a copy of its ring."""
    from dronerl_amd.dqn import ConvQNetwork, LargeBatchConvDQNLearner, ReplayBuffer
    W, conv, dense = NETS[name]
    nc, out = len(conv), []
    for hp, (ow, ob), (tw, tb) in zip(hps, online, target):
        net = ConvQNetwork((W, W, 6), conv, dense, input="code")
        net.load(ow[:nc], ob[:nc], ow[nc:], ob[nc:])
        learner = LargeBatchConvDQNLearner(net, hp, target=(tw[:nc], tb[:nc], tw[nc:], tb[nc:]))
        out.append((learner, ReplayBuffer(cap, W * W * 6, torch.device("cuda"), code_radius=radius)))
    return out


def _assert_member_equals(pop, m, learner, where):
    for k in SETS:
        for l, ((w, b), (sw, sb)) in enumerate(zip(pop.params(k, m), learner.params(k))):
            assert torch.equal(w.view(torch.int32), sw.view(torch.int32)), (where, m, k, l, "W")
            assert torch.equal(b.view(torch.int32), sb.view(torch.int32)), (where, m, k, l, "b")
    # drl_dqn_counters' first 32 bytes: step, count, epsilon, loss, beta1_pow, beta2_pow
    lay = pop.layout.member
    mine = pop.member_block(m)[lay.counters_off:lay.counters_off + 32]
    ref = learner.block[learner.layout.counters_off:learner.layout.counters_off + 32]
    assert torch.equal(mine, ref), (where, m, pop.counters(m), learner.counters())


# The issue's shape (a ring of 96 slots, E = 5, 24 steps; net g at 8 steps): the ring never holds 130 rows, so the
# batch-130 member only schedules.  The last case (a ring of 160 slots, E = 16) is added so that three chunks train.
LEARNER_CASES = [("b", 96, 5, 24), ("c", 96, 5, 24), ("i", 96, 5, 24), ("g", 96, 5, 8), ("b", 160, 16, 12)]


@gpu
@pytest.mark.parametrize("name,cap,E,steps", LEARNER_CASES, ids=[f"{c[0]}-ring{c[1]}-E{c[2]}" for c in LEARNER_CASES])
def test_convpop_learner_equals_the_single_agent_bit_exact(name, cap, E, steps):
    """Members with batches 1, 8, 64, 65 and 130 (max_batch 130: one, two
    and three chunks, a chunk of a single row) and different learning rate,
    gamma, tau 0.6 with target interval 3, epsilon decay every step and
    sample seed.  After every step of act -> step -> add -> train each
    member's online, target, m and v sets and its counters (step, count,
    epsilon, loss, both beta powers) equal, bit for bit, those of a
    LargeBatchConvDQNLearner with the same net, initial sets and
    hyperparameters trained on a ReplayBuffer holding a copy of that member's
    ring and size.  The first steps have size < batch for the larger members
    (they only schedule), and the ring wraps."""
    hps = _learner_hps()
    P = len(hps)
    online, target = _rand_sets(name, P, 77)
    env, pop, rb = _setup(name, hps, E, cap, seed=1, online=online, target=target)
    assert pop.max_batch == 130
    refs = _single_agents(name, hps, online, target, cap, env.params.window_radius)
    loop = _Loop(env, pop, rb)
    for m, (learner, _) in enumerate(refs):  # drl_convpop_init: moments and counters from zero, epsilon_start
        _assert_member_equals(pop, m, learner, "init")
    trained = [0] * P
    for t in range(steps):
        loop.fill()
        for m, (learner, ring) in enumerate(refs):
            mine = rb.ring(m)
            for k in ("obs", "next_obs", "actions", "rewards", "dones"):
                getattr(ring, k).copy_(mine[k])
            ring.size, ring.cursor = rb.size, rb.cursor
            learner.train(ring)
        pop.train(rb)
        for m, (learner, _) in enumerate(refs):
            want = rb.size >= hps[m].batch
            assert pop.counters(m)["trained"] == int(want), (t, m)
            trained[m] += int(want)
            _assert_member_equals(pop, m, learner, f"step {t}")
    want_counts = [sum(min(E * (t + 1), cap) >= hp.batch for t in range(steps)) for hp in hps]
    assert trained == want_counts and [pop.counters(m)["count"] for m in range(P)] == want_counts
    assert want_counts[0] == steps and want_counts[1] > 0
    if steps * E > cap:  # (the 24-step cases: two chunks trained, the ring wrapped)
        assert want_counts[3] > 0 and rb.size == cap
    if cap >= 130:
        assert want_counts[4] > 0  # three chunks trained
    assert all(np.isfinite(pop.counters(m)["loss"]) for m in range(P))
    assert all(float(pop.epsilon[m]) == learner.counters()["epsilon"] for m, (learner, _) in enumerate(refs))


@gpu
def test_convpop_members_do_not_depend_on_each_other():
    """Member m of a population of three is reproduced bit for bit by a
    population of one at env_offset + m E through train_population (12 steps,
    network_type conv, a reset at step 0 and at step 10): parameters,
    counters, rings and actions.  Every population trains on a scratch it
    found full of NaNs; the guard behind the block (filled with a NaN
    pattern) and the unwritten tail of each ring (filled before the first
    train) stay untouched."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.population import train_population
    E, cap, steps, G, off = 8, 128, 12, 4096, 500
    ep = EnvParams(**SHAPES["b"])
    hps = [DQNHParams(batch=2, sample_seed=7, epsilon_decay=0.9, epsilon_decay_every=1),
           DQNHParams(batch=66, learning_rate=3e-3, tau=0.5, target_update_interval=2, sample_seed=8),
           DQNHParams(batch=7, gamma=0.7, sample_seed=9, epsilon_decay=0.5, epsilon_decay_every=2)]
    seeds = [21, 34, 55]
    PAT = 0x7FC0BEEF

    def run(members, env_offset):
        acts, tails = [], {}

        def on_step(t, pop, rb, a, rew, don):
            acts.append(_host(a))
            if t:
                return
            lay = pop.layout
            for k in range(len(members)):
                pop.member_block(k)[lay.member.scratch_off:].view(torch.int32).fill_(PAT)
                for key, v in rb.ring(k).items():  # (the slots 12 steps of E envs never reach)
                    v[steps * E:].view(torch.uint8).fill_(0xA5)
            pop._alloc[lay.bytes:].view(torch.int32).fill_(PAT)
            tails["records"] = pop._alloc[lay.hparams_off:].clone()

        res = train_population(ep, [hps[m] for m in members], E, steps, reset_env_every=10, memory_size=cap, seed=4,
                               env_offset=env_offset, seeds=[seeds[m] for m in members], on_step=on_step,
                               network_type="conv", conv_layers=NETS["b"][1], guard_bytes=G)
        assert torch.equal(res.pop._alloc[res.pop.layout.hparams_off:], tails["records"])
        for k in range(len(members)):
            for key, v in res.replay.ring(k).items():
                assert bool((v[steps * E:].view(torch.uint8) == 0xA5).all()), (k, key)
        return res.pop, res.replay, np.stack(acts)

    pop3, rb3, acts3 = run([0, 1, 2], off)
    assert [pop3.counters(m)["count"] for m in range(3)] == [12, 4, 12]
    for m in range(3):
        pop1, rb1, acts1 = run([m], off + m * E)
        for k in SETS:
            for (w, b), (w1, b1) in zip(pop3.params(k, m), pop1.params(k, 0)):
                assert torch.equal(w.view(torch.int32), w1.view(torch.int32)), (m, k)
                assert torch.equal(b.view(torch.int32), b1.view(torch.int32)), (m, k)
        c3, c1 = pop3.counters(m), pop1.counters(0)
        assert c3 == c1 and not np.isnan(c3["loss"]), (m, c3, c1)
        for k, v in rb3.ring(m).items():
            assert torch.equal(v, rb1.ring(0)[k]), (m, k)
        assert np.array_equal(acts3[:, m * E:(m + 1) * E], acts1), m


@gpu
def test_convpop_step_replays_from_a_captured_graph():
    """One captured population step -- act, the env step, the add, train --
    replayed 6 times equals 6 eager steps bit for bit: the chain is linear,
    nothing in it synchronises with the host or reads host hyperparameters.
    The host's part of a step is frozen by a capture, so both runs keep it
    fixed: the act's step argument, the ring's cursor, no refill."""
    from dronerl_amd.dqn import DQNHParams
    E, cap, k = 4, 128, 6
    hps = [DQNHParams(batch=3, sample_seed=1, epsilon_decay=0.9, epsilon_decay_every=1),
           DQNHParams(batch=70, sample_seed=2, tau=0.5, target_update_interval=2, learning_rate=3e-3)]
    online, target = _rand_sets("i", 2, 31)

    def fresh():
        env, pop, rb = _setup("i", hps, E, cap, seed=6, online=online, target=target)
        env.refill_every = 0  # (where the respawn draws happen, never what they are)
        loop = _Loop(env, pop, rb)
        for _ in range(18):  # (72 rows: both members train in every step below)
            loop.fill()
        rew = torch.empty((2 * E, env.n_drones), dtype=torch.float32, device="cuda")
        don = torch.empty((2 * E, env.n_drones), dtype=torch.uint8, device="cuda")
        q = torch.empty((2 * E, 5), device="cuda")
        c0, s0 = rb.cursor, rb.size

        def step():
            pop.act(loop.cur, 9, seed=3, actions=loop.acts, synth=(5, 9), q_out=q)
            env.step(loop.acts, rewards=rew, dones=don, code=loop.nxt)
            rb.cursor, rb.size = c0, s0
            rb.add(loop.cur, loop.acts, rew, loop.nxt, don)
            pop.train(rb)
            loop.cur.copy_(loop.nxt)
        return env, pop, rb, loop, q, step, (rew, don)

    env, pop, rb, loop, q, step, out = fresh()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    env2, pop2, rb2, loop2, q2, step2, out2 = fresh()
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
    assert torch.equal(pop.block, pop2.block)  # (parameters, counters, scratch and records alike)
    assert torch.equal(q.view(torch.int32), q2.view(torch.int32)) and torch.equal(loop.acts, loop2.acts)
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and torch.equal(loop.cur, loop2.cur)
    for key in ("obs", "next_obs", "actions", "rewards", "dones"):
        assert torch.equal(getattr(rb, key), getattr(rb2, key)), key
    d1, d2 = env.decode(), env2.decode()
    assert all(torch.equal(d1[key], d2[key]) for key in d1)
    assert [pop2.counters(m)["count"] for m in range(2)] == [k, k]
    assert pop2.counters(0)["step"] == k  # (the fills above do not train)
    assert pop2.counters(0)["epsilon"] < 0.9 ** (k - 1)  # (every replay decayed the device epsilon the next one read)


@gpu
def test_convpop_sample_slots_are_each_members_draws():
    """drl_convpop_sample_rows equals dq_sample's draws (oracle
    sample_indices) per member at each step (the device step counter) in its
    first batch_m entries, -1 behind them."""
    hps = _learner_hps()
    env, pop, rb = _setup("b", hps, 4, 50)
    loop = _Loop(env, pop, rb)
    SENT, P, B = -77, len(hps), 130
    buf = torch.full((P * B + 8,), SENT, dtype=torch.int64, device="cuda")
    for t in range(5):
        loop.fill()
        slots = _host(pop.sample_slots(rb.size, out=buf[:P * B].view(P, B)))
        for m, hp in enumerate(hps):
            want = O.sample_indices(hp.sample_seed, t, hp.batch, rb.size)
            assert slots[m, :hp.batch].tolist() == want and (slots[m, hp.batch:] == -1).all(), (t, m)
        pop.train(rb)
    assert bool((buf[P * B:] == SENT).all())


@gpu
def test_conv_sweep_cli_end_to_end(tmp_path):
    """`python -m dronerl_amd.conv_sweep` as a fresh child process: a 2 x 2
    grid x 2 seeds, E = 4, 40 steps, two short evals, checkpoints.  The table
    has 8 rows, and each checkpoint reloads (checkpoint.to_qnet) to the
    member's weights bit for bit."""
    from dronerl_amd import conv_sweep
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    argv = ["--grid", '{"learning_rate": [1e-4, 5e-4], "batch_size": [8, 16]}', "--members_seeds", "2", "--num_envs",
            "4", "--num_steps", "40", "--num_evals", "2", "--num_eval_steps", "50", "--save_final_checkpoint"]
    r = subprocess.run([sys.executable, "-m", "dronerl_amd.conv_sweep", *argv, "--output_dir", str(tmp_path)],
                       cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["members"] == 8
    table = json.load(open(out["table_path"]))["table"]
    assert len(table) == 8
    assert [(t["learning_rate"], t["batch_size"], t["seed"]) for t in table] == [
        (lr, b, s) for lr in (1e-4, 5e-4) for b in (8, 16) for s in (0, 1)]
    for t in table:
        assert t["steps"] == 40 and t["train_steps"] == 40 - (t["batch_size"] // 4 - 1)
        assert np.isfinite([t["eval_reward_mean"], t["eval_reward_std"], t["final_loss"]]).all()
        assert 0.0 < t["final_epsilon"] < 1.0
    # a second, identical run in this process: the members' weights to compare the checkpoints with
    from dronerl_amd.population import train_population
    from dronerl_amd.train import env_params_of
    args, points = conv_sweep.parse_args(argv)
    hps, seeds, _ = conv_sweep.members_of(args, points)
    res = train_population(env_params_of(args), hps, 4, 40, seeds=seeds, network_type="conv",
                           conv_layers=args.conv_layers, conv_dense_layers=tuple(args.conv_dense_layers))
    for m, t in enumerate(table):
        for fmt in ("jax", "torch"):
            net = to_qnet(read_checkpoint(t[f"checkpoint_{fmt}"]))
            got = list(zip((*net.conv_weights, *net.weights), (*net.conv_biases, *net.biases)))
            for (w, b), (nw, nb) in zip(res.pop.params("online", m), got):
                assert torch.equal(w.view(torch.int32), nw.view(torch.int32)), (m, fmt)
                assert torch.equal(b.view(torch.int32), nb.view(torch.int32)), (m, fmt)
