"""Shared-policy self-play with conv learners: K conv DQN learners, each
driving a team of M drone indices of the shared envs -- drl_convselfplay_act
(dronerl_amd/csrc/convselfplay/), dronerl_amd.selfplay.ConvSelfPlayDQN,
train_selfplay(network_type="conv") and `python -m dronerl_amd.conv_selfplay`.

Reference: torch_impl/helpers/rl_helpers.py:44-65 (MultiAgentTrainer.train
with one agent object under several keys of `agents`); each learner is
train_jax.py:38-115's learner block with network_type 'conv' on its team's
rows.

The yardsticks are code that exists without conv self-play:
tests/_conv_pop_ref.py (a numpy restatement of cl_forward's summation order),
drl_convpop_act and drl_convleague_act (both unchanged), the single-agent conv
learner (LargeBatchConvDQNLearner, as tests/test_conv_population.py uses it),
the two action hashes, the oracle env and train_league(network_type="conv").
Every GPU comparison is BIT FOR BIT: no tolerance anywhere; the learning test
asserts an ordering only."""
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
from test_conv_league import SHAPES, _np_online, _rand_sets
from test_conv_population import _assert_member_equals, _bits, _desc, _host, _single_agents
from test_dqn import _hash_explore
from test_selfplay import _stepped_codes, _team_maps
from tests import _conv_learner_ref as R
from tests import _conv_pop_ref as F32

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
MODELS = os.path.join(HERE, "golden", "sample_models")
vp = ctypes.c_void_p
ENV_TILES = (16, 8, 4, 2)
SENT = 0x5A5A5A5A
# 9x9 windows, two padded 3x3 conv layers: the forward-only rows of 4,384 and 5,680 words leave room for 8 and 4
# of them in a CU's 160 KiB (the nets of tests/_conv_learner_ref.py NETS all have 16)
SMALL_TILE_NETS = {8: (9, (R._c(16, 3, 1, 1), R._c(32, 3, 1, 1)), ()),
                   4: (9, (R._c(32, 3, 1, 1), R._c(32, 3, 1, 1)), ())}


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind, _bind_convnet
    from dronerl_amd.population import _bind_convpop, _bind_pop
    from dronerl_amd.selfplay import _bind_convselfplay
    return _bind_convselfplay(_bind_convpop(_bind_pop(_bind(_bind_convnet(lib())))))


def _map(*flat):
    return (ctypes.c_int32 * len(flat))(*flat)


def _net_desc(net):
    from dronerl_amd.dqn import convnet_desc
    W, conv, dense = net
    return convnet_desc((W, W, 6), conv, dense, 5, "code")


# ------------------------------------------------------------------- CPU ---
def test_convselfplay_act_validates_before_device_work():
    """drl_convselfplay_act is refused before any device work (no GPU), with
    the reason in drl_last_error: every check of drl_convleague_act (NULL
    descriptor, block, codes or actions; a misaligned block, codes or q;
    members 0, negative, above n_drones; n_drones 0 and 65; num_envs 0,
    negative and num_envs * n_drones at 2^31; an f32-input descriptor; window
    3; 9 actions; max_batch 0) and every check of the map (NULL, team < 1,
    members * team > n_drones, an index outside [0, n_drones), an index named
    twice)."""
    from dronerl_amd.dqn import convnet_desc
    L = _lib()
    E = L.drl_last_error
    good = _desc("b")
    blk, ptr = vp(1 << 20), vp(1 << 21)
    odd = vp((1 << 21) + 8)
    w3 = convnet_desc((3, 3, 6), (R._c(8, 1, 1, 0),), (8,), 5, "code")
    ident = _map(0, 1, 2, 3)

    def act(d=good, K=2, B=8, pop=blk, codes=ptr, E_=4, dr=ident, M=2, acts=ptr, N=4, q=None):
        return L.drl_convselfplay_act(None if d is None else ctypes.byref(d), K, B, pop, codes, E_, dr, M, 0, 0, 0, 0,
                                      acts, N, q, None)

    assert act(d=None) != 0 and b"NULL" in E()
    # the map
    assert act(dr=None) != 0 and b"drones" in E() and b"NULL" in E()
    assert act(M=0) != 0 and b"team must be >= 1" in E()
    assert act(M=-1) != 0 and b"team must be >= 1" in E()
    assert act(K=2, M=3, N=4) != 0 and b"members * team" in E()
    assert act(K=1, M=5, N=4) != 0 and b"members * team" in E()
    assert act(K=2, M=1 << 30, N=4) != 0 and b"members * team" in E()
    assert act(dr=_map(0, 1, 2, 4)) != 0 and b"outside [0, n_drones)" in E()
    assert act(dr=_map(0, -1, 2, 3)) != 0 and b"outside [0, n_drones)" in E()
    assert act(dr=_map(3, 1, 3, 0)) != 0 and b"named twice" in E()
    assert act(dr=_map(2, 2), K=1, M=2) != 0 and b"named twice" in E()
    # drl_convleague_act's checks
    for K, N in ((0, 4), (-1, 4), (5, 4), (65, 64), (2, 1)):
        assert act(K=K, M=1, N=N) != 0 and b"members" in E(), (K, N, E())
    assert act(N=0) != 0 and b"n_drones" in E()
    assert act(N=65) != 0 and b"n_drones" in E()
    assert act(E_=0) != 0 and b"num_envs" in E()
    assert act(E_=-3) != 0 and b"num_envs" in E()
    assert act(E_=1 << 29) != 0 and b"num_envs" in E()
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


def _layout_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("cvs") / "convselfplay_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "convselfplay_layout_check.cpp")], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_convselfplay_row_map_takes_every_row_once(tmp_path_factory):
    """tests/native/convselfplay_layout_check.cpp, a stand-alone program under
    the address and undefined-behaviour sanitizers (nothing is loaded into
    Python): over T {16, 8, 4, 2} x E {1, 2, T - 1, T, T + 1, 3 T + 5} x M {1,
    2, 3, 6} x K {1, 2} every row of every learner is taken by exactly one
    (workgroup, tile lane), no tile holds rows of two learners, the lanes past
    M * E are inactive, and the gathered source of a row and its action and Q
    destinations equal a row-by-row loop's; tiles that hold rows of several
    drones, ragged last tiles and a team of six in one tile all occur.  Its
    sweep of descriptors finds env tiles 16, 8 and 4 and none of 2; the plan
    query the Python layer reads gives the two 9x9 nets of the small-tile test
    the tiles the header gives the kernel, 8 and 4."""
    from dronerl_amd.league import conv_act_plan
    r = _layout_check(tmp_path_factory)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    m = re.search(r"cases (\d+): tiles of several drones (\d+), ragged tiles (\d+), a team of six in one tile (\d+)",
                  r.stdout)
    assert m and int(m.group(1)) == 4 * 6 * 4 * 2 and all(int(v) > 0 for v in m.groups()), r.stdout
    t = re.search(r"TILES 16:(\d+) 8:(\d+) 4:(\d+) 2:(\d+)", r.stdout)
    assert t and int(t.group(1)) > 0 and int(t.group(2)) > 0 and int(t.group(3)) > 0 and int(t.group(4)) == 0, r.stdout
    assert "NET 9x9-16-32 : 8" in r.stdout and "NET 9x9-32-32 : 4" in r.stdout
    for T, net in SMALL_TILE_NETS.items():
        assert conv_act_plan(_net_desc(net))["env_tile"] == T
    for name in ("a", "b", "c", "f", "g", "h", "i"):
        assert conv_act_plan(_desc(name))["env_tile"] == 16, name


# Every __global__ kernel under csrc/convselfplay/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_convselfplay_act_kernel": "test_conv_selfplay.py::test_convselfplay_act_is_the_learners_forward_bit_exact",
}


def test_every_convselfplay_kernel_has_a_gpu_test():
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "convselfplay", "*.hip")):
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


def test_conv_selfplay_cli_maps_grid_and_refusals():
    """conv_selfplay.parse_args: --drones maps to the [K][M] list and the
    default map is k * M + j; the grid maps to learners (K points or one
    shared); --opponents' plain words take the drone indices no team holds;
    the conv options arrive; every refusal carries its reason (dense names
    dronerl_amd.selfplay).  dronerl_amd.selfplay keeps refusing conv and names
    this command too; train_selfplay refuses an unknown network_type."""
    from dronerl_amd import EnvParams, conv_selfplay, selfplay
    from dronerl_amd.league import learners_of
    with pytest.raises(ValueError, match="conv learners only.*python -m dronerl_amd.selfplay"):
        conv_selfplay.parse_args(["--network_type", "dense"])
    with pytest.raises(ValueError, match="one GPU.*use_sharding.*dronerl_amd.train"):
        conv_selfplay.parse_args(["--use_sharding", "--num_envs", "8"])
    with pytest.raises(ValueError, match="more team drones than drones"):
        conv_selfplay.parse_args(["--learners", "2", "--drones_per_learner", "3", "--n_drones", "5"])
    with pytest.raises(ValueError, match="opponent index 2 is inside learner 0's team"):
        conv_selfplay.parse_args(["--learners", "1", "--drones_per_learner", "2", "--n_drones", "4", "--drones", "0,2",
                                  "--opponents", "2=a.safetensors"])
    with pytest.raises(ValueError, match="named twice"):
        conv_selfplay.parse_args(["--drones_per_learner", "2", "--drones", "1,1"])
    with pytest.raises(ValueError, match="drone indices 0..3"):
        conv_selfplay.parse_args(["--drones_per_learner", "2", "--drones", "1,4", "--n_drones", "4"])
    with pytest.raises(ValueError, match="names 3 drone indices.*need 4"):
        conv_selfplay.parse_args(["--learners", "2", "--drones_per_learner", "2", "--drones", "0,1,2", "--n_drones", "6"])
    with pytest.raises(ValueError, match="comma-separated"):
        conv_selfplay.parse_args(["--drones", "0;1"])
    with pytest.raises(ValueError, match="must be >= 1"):
        conv_selfplay.parse_args(["--drones_per_learner", "0"])
    with pytest.raises(ValueError, match="must be >= 1"):
        conv_selfplay.parse_args(["--learners", "0"])
    with pytest.raises(ValueError, match="do not fit"):
        conv_selfplay.parse_args(["--drones_per_learner", "3", "--n_drones", "4", "--opponents", "a", "b"])
    with pytest.raises(ValueError, match="not valid JSON"):
        conv_selfplay.parse_args(["--grid", "{gamma: 1}"])
    with pytest.raises(ValueError, match="2 points: one per learner .1. or one shared"):
        conv_selfplay.parse_args(["--grid", '{"gamma": [0.9, 0.8]}'])
    with pytest.raises(ValueError, match="self-play learners are dense nets.*dronerl_amd.conv_selfplay"):
        selfplay.parse_args(["--network_type", "conv"])
    with pytest.raises(ValueError, match="network_type"):
        selfplay.train_selfplay(EnvParams(), [], 1, 1, 1, network_type="nope")
    args, points = conv_selfplay.parse_args([
        "--learners", "1", "--drones_per_learner", "4", "--n_drones", "6", "--grid_size", "11", "--num_envs", "4096",
        "--drones", "0,2,4,5", "--opponents", "a.st", "--save_final_checkpoint"])
    assert args.drones == [[0, 2, 4, 5]] and (args.learners, args.drones_per_learner, args.num_envs) == (1, 4, 4096)
    assert args.opponents == {1: "a.st"} and points == [{}] and args.save_final_checkpoint  # (drone 3 is random)
    assert args.network_type == "conv" and len(args.conv_layers) == 1 and args.conv_layers[0]["out_channels"] == 8
    a2, p2 = conv_selfplay.parse_args([
        "--learners", "2", "--drones_per_learner", "3", "--n_drones", "8", "--grid", '{"learning_rate": [1e-4, 5e-4]}',
        "--opponents", "7=x.st", "random", "--seed", "5", "--gamma", "0.8", "--network_type", "conv", "--conv_layers",
        '[{"out_channels": 16, "kernel_size": 3, "padding": 1}, {"out_channels": 32, "kernel_size": 3, "padding": 1}]',
        "--conv_dense_layers", "128", "64"])
    assert a2.drones == [[0, 1, 2], [3, 4, 5]] == selfplay.default_drones(2, 3)
    assert a2.opponents == {6: None, 7: "x.st"}
    hps = learners_of(a2, p2)
    assert [hp.learning_rate for hp in hps] == [1e-4, 5e-4] and all(hp.gamma == 0.8 for hp in hps)
    assert [hp.sample_seed for hp in hps] == [5, 6]
    assert [c["out_channels"] for c in a2.conv_layers] == [16, 32] and tuple(a2.conv_dense_layers) == (128, 64)
    a3, _ = conv_selfplay.parse_args(["--learners", "2", "--drones_per_learner", "2", "--n_drones", "5", "--drones",
                                      "4,1,0,3"])
    assert a3.drones == [[4, 1], [0, 3]] and a3.opponents == {}
    a4, _ = conv_selfplay.parse_args([])
    assert (a4.learners, a4.drones_per_learner, a4.drones, a4.network_type) == (1, 2, [[0, 1]], "conv")


# ------------------------------------------------------------------- GPU ---
def _gathered(codes, drones):
    """codes [N, E, CB] -> the teams' rows [K * M * E, CB] in (learner, team slot, env) order."""
    return torch.cat([codes[dr] for row in drones for dr in row]).contiguous()


@gpu
@pytest.mark.parametrize("which", [0, 1, 2], ids=["one-learner-every-drone", "two-teams-permuted", "three-descending"])
@pytest.mark.parametrize("name", ["b", "c", "g", "i", "h"])
def test_convselfplay_act_is_the_learners_forward_bit_exact(name, which):
    """K learners with different random weights and biases on teams of M
    drones, at E = 1, T - 1, T, T + 1 and 3 T + 5 envs (T = 16 for these nets,
    from the plan query; with M >= 2 tile edges fall inside and across team
    slots and the last tile is ragged), three random env steps in, every
    learner in turn at epsilon 0, 1 and 0.3: learner k's Q of team slot j and
    env i equals tests/_conv_pop_ref.forward on the decoded row
    codes[drones[k][j]][i] bit for bit, laid out [K][M][E][A], and equals
    drl_convpop_act's q_out on the same gathered K * M * E rows (a
    ConvPopulationDQN with the same weights and M * E envs per member) bit for
    bit; the action in column drones[k][j] is the explore draw of the stream
    seed + drone index or the first argmax of that Q; the action matrix was
    filled with a sentinel and Q with NaN: the columns of drones in no team
    keep it, as do the 64 words behind both buffers; the greedy flag ignores
    epsilon."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import conv_act_plan
    from dronerl_amd.population import ConvPopulationDQN
    from dronerl_amd.selfplay import ConvSelfPlayDQN
    W, conv, dense = R.NETS[name]
    ep = EnvParams(**SHAPES[name])
    N, A = ep.n_drones, 5
    K, M, drones = _team_maps(N)[which]
    T = conv_act_plan(_desc(name))["env_tile"]
    assert T == 16
    EPS = [0.0, 1.0, 0.3]
    hps = [DQNHParams(batch=8, epsilon_decay=1.0, epsilon_end=0.0)] * K
    online, target = _rand_sets(name, K, 13)
    free = [d for d in range(N) if d not in {x for row in drones for x in row}]
    for E in (1, T - 1, T, T + 1, 3 * T + 5):
        env, codes = _stepped_codes(ep, E)
        lg = ConvSelfPlayDQN((W, W, 6), conv, dense, hps, E, drones=drones, online=online, target=target)
        assert lg.team == M and lg.drones == drones and lg.act_plan["env_tile"] == T
        abuf = torch.full((E * N + 64,), SENT, dtype=torch.int32, device="cuda")
        qbuf = torch.full((K * M * E * A + 64,), float("nan"), dtype=torch.float32, device="cuda")
        acts, q = abuf[:E * N].view(E, N), qbuf[:K * M * E * A].view(K, M, E, A)
        c_h = _host(codes)
        want = [[F32.forward(_np_online(lg, k), conv, O.decode_code_rows(c_h[drones[k][j]], W), W) for j in range(M)]
                for k in range(K)]
        # drl_convpop_act (unchanged) on the same rows: a population of K members with M * E envs each
        pop = ConvPopulationDQN((W, W, 6), conv, dense, hps, M * E, online=online, target=target)
        qpop = torch.full((K * M * E, A), float("nan"), dtype=torch.float32, device="cuda")
        pop.act(_gathered(codes, drones), 6, seed=3, q_out=qpop)
        qpop_h = _bits(_host(qpop)).reshape(K, M, E, A)
        for s in range(3):
            eps = [EPS[(k + s) % 3] for k in range(K)]
            lg.epsilon.copy_(torch.tensor(eps, dtype=torch.float32))
            abuf.fill_(SENT)
            qbuf.fill_(float("nan"))
            lg.act(codes, 6, seed=3, env_offset=env.env_offset, actions=acts, q=q)
            a_h, q_h = _host(acts), _host(q)
            assert np.array_equal(_bits(q_h), qpop_h), ("convpop Q", E, s)
            for k in range(K):
                for j, dr in enumerate(drones[k]):
                    assert np.array_equal(_bits(q_h[k, j]), _bits(want[k][j])), ("Q", E, k, j)
                    for i in range(E):
                        explore, rnd = _hash_explore(3 + dr, 6, 1000 + i, A, eps[k])
                        assert a_h[i, dr] == (rnd if explore else int(np.argmax(want[k][j][i]))), (E, s, k, j, i)
            assert (a_h[:, free] == SENT).all(), E
            assert bool((abuf[E * N:] == SENT).all()) and bool(torch.isnan(qbuf[K * M * E * A:]).all()), E
        # greedy: the argmax everywhere, whatever epsilon holds; no Q buffer
        lg.epsilon.fill_(1.0)
        abuf.fill_(SENT)
        lg.act(codes, 6, seed=3, env_offset=env.env_offset, actions=acts, greedy=True)
        g_h = _host(acts)
        for k in range(K):
            for j, dr in enumerate(drones[k]):
                assert np.array_equal(g_h[:, dr], np.argmax(want[k][j], axis=1).astype(np.int32)), ("greedy", E, k, j)
        assert (g_h[:, free] == SENT).all() and bool((abuf[E * N:] == SENT).all()), E


@gpu
@pytest.mark.parametrize("T", sorted(SMALL_TILE_NETS, reverse=True), ids=["tile-8", "tile-4"])
def test_convselfplay_act_on_the_smaller_tiles(T):
    """The tiles below 16 (no net of tests/_conv_learner_ref.py NETS reaches
    them): 9x9 windows and two padded 3x3 conv layers of 16 then 32 channels
    (T = 8) and of 32 then 32 (T = 4), the plan query asserted.  Two learners
    with different random parameters on the permuted teams [[6, 1], [4, 3]] of
    eight drones at E = T + 1 and 3 T + 5: Q [K][M][E][A] and the greedy
    actions equal drl_convpop_act's on the gathered rows (a ConvPopulationDQN
    with the same weights and M * E envs per member) bit for bit; the other
    columns and the 64 words behind both buffers keep their sentinels.  T = 2
    has no case: the layout checker's sweep of the descriptors cg::plan accepts
    at windows up to 9 (tests/native/convselfplay_layout_check.cpp) finds
    none that yields it -- a forward-only row above 40 KB goes with a learner
    row above the 64 KB cg::plan allows."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import conv_act_plan
    from dronerl_amd.population import ConvPopulationDQN
    from dronerl_amd.selfplay import ConvSelfPlayDQN
    net = SMALL_TILE_NETS[T]
    W, conv, dense = net
    assert conv_act_plan(_net_desc(net))["env_tile"] == T
    ep = EnvParams(**SHAPES["c"])
    N, A = ep.n_drones, 5
    K, M, drones = _team_maps(N)[1]
    assert (K, M, drones) == (2, 2, [[6, 1], [4, 3]])
    hps = [DQNHParams(batch=8, epsilon_start=0.3, epsilon_decay=1.0, epsilon_end=0.0)] * K

    def one(s):
        ws, bs = zip(*R.random_params(W, conv, dense, s))
        return [torch.tensor(w) for w in ws], [torch.tensor(b) for b in bs]
    online, target = [one(13 + 2 * k) for k in range(K)], [one(14 + 2 * k) for k in range(K)]
    free = [d for d in range(N) if d not in {x for row in drones for x in row}]
    for E in (T + 1, 3 * T + 5):
        env, codes = _stepped_codes(ep, E)
        lg = ConvSelfPlayDQN((W, W, 6), conv, dense, hps, E, drones=drones, online=online, target=target)
        assert lg.act_plan["env_tile"] == T
        pop = ConvPopulationDQN((W, W, 6), conv, dense, hps, M * E, online=online, target=target)
        qpop = torch.full((K * M * E, A), float("nan"), dtype=torch.float32, device="cuda")
        apop = pop.act(_gathered(codes, drones), 6, seed=3, q_out=qpop, greedy=True)
        abuf = torch.full((E * N + 64,), SENT, dtype=torch.int32, device="cuda")
        qbuf = torch.full((K * M * E * A + 64,), float("nan"), dtype=torch.float32, device="cuda")
        acts, q = abuf[:E * N].view(E, N), qbuf[:K * M * E * A].view(K, M, E, A)
        lg.act(codes, 6, seed=3, env_offset=env.env_offset, actions=acts, q=q, greedy=True)
        assert not bool(torch.isnan(q).any())
        assert torch.equal(q.reshape(K * M * E, A).view(torch.int32), qpop.view(torch.int32)), ("Q", E)
        a_h, want = _host(acts), _host(apop[:, 0]).reshape(K, M, E)
        for k in range(K):
            for j, dr in enumerate(drones[k]):
                assert np.array_equal(a_h[:, dr], want[k, j]), ("greedy", E, k, j)
        assert (a_h[:, free] == SENT).all(), E
        assert bool((abuf[E * N:] == SENT).all()) and bool(torch.isnan(qbuf[K * M * E * A:]).all()), E


@gpu
@pytest.mark.parametrize("K", [1, 3, "N"])
@pytest.mark.parametrize("name", ["b", "c", "g", "i", "h"])
def test_convselfplay_team_of_one_is_the_conv_league_act(name, K):
    """Teams of one on the identity map (learner k on drone k) against
    ConvLeagueDQN.act on the same block, codes, seed and step, at the act
    test's envs: the action buffers (sentinel columns included) and Q are
    byte-equal, exploring and greedy."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import ConvLeagueDQN, conv_act_plan
    from dronerl_amd.selfplay import ConvSelfPlayDQN
    W, conv, dense = R.NETS[name]
    ep = EnvParams(**SHAPES[name])
    N, A = ep.n_drones, 5
    K = N if K == "N" else K
    T = conv_act_plan(_desc(name))["env_tile"]
    eps = ([0.0, 1.0, 0.3, 0.7] * 2)[:K]
    hps = [DQNHParams(batch=8, epsilon_start=e, epsilon_decay=1.0, epsilon_end=0.0) for e in eps]
    online, target = _rand_sets(name, K, 13)
    for E in (1, T - 1, T, T + 1, 3 * T + 5):
        env, codes = _stepped_codes(ep, E)
        kw = dict(online=online, target=target)
        sp = ConvSelfPlayDQN((W, W, 6), conv, dense, hps, E, **kw)
        lg = ConvLeagueDQN((W, W, 6), conv, dense, hps, E, **kw)
        assert sp.drones == [[k] for k in range(K)] and sp.team == 1
        for greedy in (False, True):
            bufs = []
            for net, qshape in ((sp, (K, 1, E, A)), (lg, (K, E, A))):
                acts = torch.full((E, N), SENT, dtype=torch.int32, device="cuda")
                q = torch.full(qshape, float("nan"), dtype=torch.float32, device="cuda")
                net.act(codes, 6, seed=3, env_offset=env.env_offset, actions=acts, q=q, greedy=greedy)
                bufs.append((acts, q.view(K, E, A).view(torch.int32)))
            assert torch.equal(bufs[0][0], bufs[1][0]), ("actions", E, greedy)
            assert torch.equal(bufs[0][1], bufs[1][1]), ("Q", E, greedy)


@gpu
def test_train_conv_selfplay_matches_a_host_loop():
    """train_selfplay(network_type="conv") (net i; K = 2 learners with
    different hyperparameters on the permuted teams [[4, 1], [0, 3]], drone 2
    random, N = 5, E = 3, 12 steps, reset_env_every 5, capacity 20: six rows
    per step, the ring wraps at step 3) against a host loop built from the
    oracle env, tests/_conv_pop_ref.forward plus the two hashes for the
    actions, numpy rings filled row by row, and per learner the single-agent
    conv learner (LargeBatchConvDQNLearner, ONE train per env step) on a copy
    of the ring: actions, rewards and dones every step; the rings after every
    add (their codes decode to the oracle env's windows); at the end every
    learner's four parameter sets and counters, the rings, the cursor and the
    size."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.selfplay import ConvSelfPlayDQN, train_selfplay
    from oracle.oracle import OracleEnv, Params, synth_actions
    K, M, E, steps, cap, seed, aseed, sseed = 2, 2, 3, 12, 20, 3, 7, 2024
    drones = [[4, 1], [0, 3]]
    W, conv, dense = R.NETS["i"]
    ep = EnvParams(n_drones=5, grid_size=9, window_radius=3)
    D, A, N = W * W * 6, 5, 5
    hps = [DQNHParams(batch=4, num_steps=steps, sample_seed=1, target_update_interval=2),
           DQNHParams(batch=9, num_steps=steps, sample_seed=2, learning_rate=3e-3, tau=0.5, gamma=0.8,
                      epsilon_end=0.2, epsilon_decay_every=2)]
    seen = []

    def on_step(t, lg, rb, acts, rew, don):  # (between the add and the train of step t)
        seen.append((_host(acts), _host(rew), _host(don), [{k: v.clone() for k, v in rb.ring(m).items()} for m in range(K)],
                     rb.cursor, rb.size))

    res = train_selfplay(ep, hps, M, E, steps, drones=drones, reset_env_every=5, memory_size=cap, seed=seed,
                         act_seed=aseed, action_seed=sseed, seeds=[5, 9], on_step=on_step, network_type="conv",
                         conv_layers=conv, conv_dense_layers=dense)
    assert isinstance(res.league, ConvSelfPlayDQN) and res.league.drones == drones
    # ---- the host loop ----
    init = ConvSelfPlayDQN((W, W, 6), conv, dense, hps, E, drones=drones, seeds=[5, 9])  # (never trained)
    sets = {which: [tuple([t.detach().cpu().clone() for t in half] for half in zip(*init.params(which, k)))
                    for k in range(K)] for which in ("online", "target")}
    refs = _single_agents("i", hps, sets["online"], sets["target"], cap, ep.window_radius)
    envs = []
    for g in range(E):
        e = OracleEnv(Params(side=9, n_drones=N))
        e.seed(seed + g)
        e.reset()
        envs.append(e)
    rings = [dict(obs=np.zeros((cap, D), np.float32), next_obs=np.zeros((cap, D), np.float32),
                  actions=np.zeros(cap, np.int32), rewards=np.zeros(cap, np.float32), dones=np.zeros(cap, np.uint8))
             for _ in range(K)]
    cursor = size = 0

    def all_obs():  # [N][E][D]: every drone index's window of every env
        o = np.stack([e.obs(3, N).reshape(N, D) for e in envs])
        return np.ascontiguousarray(o.transpose(1, 0, 2))

    obs = all_obs()
    assert len(seen) == steps
    explored = 0
    for t in range(steps):
        acts = synth_actions(sseed, t, np.arange(E), N)
        for k, (learner, _) in enumerate(refs):
            ps = [(_host(w), _host(b)) for w, b in learner.params("online")]
            eps = learner.counters()["epsilon"]
            for dr in drones[k]:
                q = F32.forward(ps, conv, obs[dr], W)
                for i in range(E):
                    explore, rnd = _hash_explore(aseed + dr, t, i, A, eps)
                    explored += int(explore)
                    acts[i, dr] = rnd if explore else int(np.argmax(q[i]))
        rew, don = np.zeros((E, N), np.float32), np.zeros((E, N), np.uint8)
        for g, e in enumerate(envs):
            r, d = e.step(acts[g])
            rew[g], don[g] = r.astype(np.float32), d
        nxt = all_obs()
        for k in range(K):
            cur = cursor
            for dr in drones[k]:
                for i in range(E):
                    rings[k]["obs"][cur], rings[k]["next_obs"][cur] = obs[dr, i], nxt[dr, i]
                    rings[k]["actions"][cur], rings[k]["rewards"][cur], rings[k]["dones"][cur] = acts[i, dr], rew[i, dr], don[i, dr]
                    cur = (cur + 1) % cap
        cursor, size = (cursor + M * E) % cap, min(size + M * E, cap)
        ga, gr, gd, grings, gcur, gsize = seen[t]
        assert np.array_equal(acts, ga), ("actions", t)
        assert np.array_equal(_bits(rew), _bits(gr)) and np.array_equal(don, gd), ("rewards/dones", t)
        assert (gcur, gsize) == (cursor, size), t
        for k, (learner, ring) in enumerate(refs):
            got = {key: _host(v) for key, v in grings[k].items()}
            for key in ("obs", "next_obs"):  # (an empty slot is a zero code row, which decodes to zeros)
                assert np.array_equal(_bits(O.decode_code_rows(got[key], W)), _bits(rings[k][key])), (t, k, key)
            assert np.array_equal(got["actions"], rings[k]["actions"]) and np.array_equal(got["dones"], rings[k]["dones"])
            assert np.array_equal(_bits(got["rewards"]), _bits(rings[k]["rewards"])), (t, k)
            for key in ("obs", "next_obs", "actions", "rewards", "dones"):
                getattr(ring, key).copy_(grings[k][key])
            ring.size, ring.cursor = size, cursor
            learner.train(ring)
        obs = nxt
        if t % 5 == 0:
            for e in envs:
                e.reset()
            obs = all_obs()
    assert 0 < explored < K * M * E * steps  # (both branches of the action rule were taken)
    assert steps * M * E > cap and size == cap  # (the ring wrapped)
    for k, (learner, _) in enumerate(refs):
        _assert_member_equals(res.league, k, learner, "end")
        for key, v in res.replay.ring(k).items():
            assert torch.equal(v, seen[-1][3][k][key]), (k, key)
    assert (res.replay.cursor, res.replay.size) == (cursor, size) == (steps * M * E % cap, cap)
    assert [res.league.counters(k)["count"] for k in range(K)] == [12, 11]  # (size >= batch: 6 rows after step 0)
    assert res.rows_per_s > 0


@gpu
def test_conv_selfplay_of_singletons_is_the_conv_league():
    """train_selfplay(drones_per_learner=1, network_type="conv") against
    train_league(network_type="conv") with the same seeds (net b, K = 2,
    N = 4, 9x9, E = 3, capacity 20, 15 steps): every step's actions, rewards
    and dones, and at the end the block (parameters, Adam state, counters,
    scratch, records), the counters, the rings, the cursor and the size, are
    bit-identical."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import train_league
    from dronerl_amd.selfplay import train_selfplay
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)
    hps = [DQNHParams(batch=4, num_steps=15, sample_seed=3, target_update_interval=2, epsilon_decay_every=1),
           DQNHParams(batch=6, num_steps=15, sample_seed=4, tau=0.5, learning_rate=3e-3, epsilon_decay_every=1)]
    kw = dict(reset_env_every=6, memory_size=20, seed=4, env_offset=40, action_seed=11, act_seed=5, seeds=[9, 10],
              network_type="conv", conv_layers=R.NETS["b"][1], conv_dense_layers=())
    got, want = [], []
    a = train_selfplay(ep, hps, 1, 3, 15, on_step=lambda t, p, rb, ac, rw, dn: got.append([_host(v) for v in (ac, rw, dn)]), **kw)
    b = train_league(ep, hps, 3, 15, on_step=lambda t, p, rb, ac, rw, dn: want.append([_host(v) for v in (ac, rw, dn)]), **kw)
    assert len(got) == len(want) == 15
    for t, (x, y) in enumerate(zip(got, want)):
        assert all(u.shape == v.shape and u.tobytes() == v.tobytes() for u, v in zip(x, y)), t
    assert torch.equal(a.league.block, b.league.block)
    for k in range(2):
        assert a.league.counters(k) == b.league.counters(k) and a.league.counters(k)["count"] > 0
        for key, v in a.replay.ring(k).items():
            assert torch.equal(v, b.replay.ring(k)[key]), (k, key)
    assert (a.replay.cursor, a.replay.size) == (b.replay.cursor, b.replay.size)


@gpu
def test_conv_selfplay_step_replays_from_a_captured_graph():
    """One captured self-play step -- synthetic columns, the conv self-play
    act, a fixed dense net's act, the env step, every drone's code, the add,
    train -- replayed 6 times equals 6 eager steps (K = 2 teams of M = 2 on
    N = 6, net b, E = 40, capacity 200: the captured add wraps the ring):
    block, rings, actions, rewards, dones and env state bit-identical.  The
    host's part of a step is frozen by a capture, so both runs keep it fixed:
    the act's step argument, the ring's cursor, no refill.  The process keeps
    its default number of hardware queues."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.evaluator import obs_code_all
    from dronerl_amd.selfplay import ConvSelfPlayDQN, SelfPlayLoop, SelfPlayReplay, resolve_team_opponents
    E, cap, k, K, M, N = 40, 200, 6, 2, 2, 6
    W, conv, dense = R.NETS["b"]
    drones = [[4, 1], [0, 3]]  # (drone 2: a fixed net; drone 5: random)
    hps = [DQNHParams(batch=3, sample_seed=1, epsilon_decay=0.9, epsilon_decay_every=1),
           DQNHParams(batch=12, sample_seed=2, tau=0.5, target_update_interval=2, learning_rate=3e-3)]
    online, target = _rand_sets("b", K, 31)
    ep = EnvParams(n_drones=N, grid_size=9, window_radius=3)
    path = {2: os.path.join(MODELS, "dqn-agent-2.safetensors")}

    def fresh():
        env = BatchedDeliveryDrones(ep, E)
        env.reset(seed=6)
        lg = ConvSelfPlayDQN((W, W, 6), conv, dense, hps, E, drones=drones, online=online, target=target)
        rb = SelfPlayReplay(K, cap, ep.window_radius)
        env.refill_every = 0  # (where the respawn draws happen, never what they are)
        loop = SelfPlayLoop(env, lg, rb, resolve_team_opponents(path, drones, ep, env.device), action_seed=5, act_seed=3)
        assert loop.any_random
        loop.step(0)
        loop.step(1)  # (back on code buffer 0; the fixed net's act has run once before the capture)
        c0, s0 = rb.cursor, rb.size
        cur, nxt = loop.codes[0], loop.codes[1]

        def step():
            loop.cur = 0
            loop.act(9)
            env.step(loop.actions, rewards=loop.rewards, dones=loop.dones)
            obs_code_all(env, nxt)
            rb.cursor, rb.size = c0, s0
            loop.add(nxt)
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
    assert (rb2.cursor, rb2.size) == (3 * M * E % cap, cap) == (40, 200)  # (the captured add wraps the ring)
    assert [lg2.counters(m)["count"] for m in range(K)] == [k + 2, k + 2]
    assert lg2.counters(0)["epsilon"] < 0.9 ** k  # (every replay decayed the device epsilon the next one read)


@gpu
def test_conv_selfplay_learner_beats_the_random_drones():
    """One conv learner (train_jax's default conv net) on drones 0 and 1 of
    four, 9x9, 4,096 envs, 300 steps at batch 256; in evaluate_selfplay's
    greedy table (5 episodes of 1,000 steps) each team drone's mean episode
    reward is above each random drone's.  The condition is the ordering
    only.  Measured on an MI355X (the run is deterministic): team drones
    -61.4 and -62.5, random drones -183.8 and -183.2 per 1,000-step
    episode."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.selfplay import ConvSelfPlayDQN, evaluate_selfplay, train_selfplay
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)
    res = train_selfplay(ep, [DQNHParams(batch=256, num_steps=300, sample_seed=0)], 2, 4096, 300, seeds=[0],
                         network_type="conv")
    assert isinstance(res.league, ConvSelfPlayDQN)
    assert res.league.counters(0)["count"] == 300 and res.replay.size == 100_000
    ev = evaluate_selfplay(res, num_steps=1000)
    print("conv self-play eval, mean episode reward per drone:", [round(float(v), 2) for v in ev["mean"]], ev["roles"])
    assert ev["scores"].shape == (5, 4) and ev["roles"] == ["learner 0", "learner 0", "random", "random"]
    for d in (0, 1):
        for o in (2, 3):
            assert float(ev["mean"][d]) > float(ev["mean"][o]), ev["mean"]


@gpu
def test_conv_selfplay_cli_end_to_end(tmp_path, capsys):
    """One conv learner (4 x 3 x 3 + dense 8) on drones 3 and 0 against the
    conv sample baseline and a random drone on a tiny run: the JSON line
    parses, roles and train counts are right, the checkpoint (two formats) is
    written and reloads through checkpoint.to_qnet as a conv net of that
    shape."""
    from dronerl_amd import conv_selfplay
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import ConvQNetwork
    out = conv_selfplay.main(["--learners", "1", "--drones_per_learner", "2", "--drones", "3,0", "--opponents",
                              os.path.join(MODELS, "dqn-agent-5.safetensors"), "--n_drones", "4", "--grid_size", "9",
                              "--num_envs", "8", "--num_steps", "30", "--conv_layers",
                              '[{"out_channels": 4, "kernel_size": 3, "padding": 1}]', "--conv_dense_layers", "8",
                              "--num_evals", "2", "--num_eval_steps", "50", "--save_final_checkpoint", "--output_dir",
                              str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["learners"] == 1 and line["drones"] == [[3, 0]] and line["replay_rows_per_sec"] > 0
    assert line["network_type"] == "conv" and line["conv_dense_layers"] == [8]
    assert [c["out_channels"] for c in line["conv_layers"]] == [4]
    assert [r["role"] for r in line["eval"]] == ["learner 0", "opponent", "random", "learner 0"]
    assert all(np.isfinite([r["reward_mean"], r["reward_std"]]).all() for r in line["eval"])
    assert [r.get("train_steps") for r in line["eval"]] == [30, None, None, 30]
    assert len(out["checkpoints"]) == 1
    for fmt in ("jax", "torch"):
        net = to_qnet(read_checkpoint(out["checkpoints"][0][fmt]))
        assert isinstance(net, ConvQNetwork), fmt
        assert [tuple(w.shape) for w in net.conv_weights] == [(4, 6, 3, 3)], fmt
        assert [tuple(w.shape) for w in net.weights] == [(8, 196), (5, 8)], fmt
        assert all(bool(torch.isfinite(w).all()) for w in (*net.conv_weights, *net.weights))
