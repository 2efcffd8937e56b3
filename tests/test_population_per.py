"""Prioritized replay for a population of dense DQN agents: drl_pop_per_*
(dronerl_amd/csrc/perpop/), population.PrioritizedPopulationReplay,
population.PrioritizedPopulationDQN, train_population(per=...) and
`python -m dronerl_amd.per_sweep`.

What pins it:
  * the single agent: a member's tree, draw, weights, step and priorities
    equal dqn.PrioritizedDQNLearner + dqn.PrioritizedReplay on the same ring
    rows BIT FOR BIT (both run the bodies of csrc/per/dronerl_per_chain.h);
  * tests/_per_ref.py and oracle/dqn_learner.py, where no single agent
    exists (hidden widths above 128) and for alpha = 0, beta = 0;
  * a population of one, for independence from the other members.
"""
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

import test_population as TP
import test_prioritized_replay as TR
from tests import _per_ref as R

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SETS = ("online", "target", "m", "v")
F = np.float32
vp = ctypes.c_void_p
_host, _bits = TR._host, TR._bits


def _lib():
    from dronerl_amd.population import _bind_pop_per
    return _bind_pop_per(TP._lib())


# ------------------------------------------------------------------- CPU ---
def test_pop_per_layout_query():
    """Host only: the member layout equals drl_per_layout_query(capacity,
    max_batch) field for field; the stride and the records' offset are
    multiples of 16; the records lie behind the last member."""
    from dronerl_amd.dqn import DrlPerLayout
    from dronerl_amd.population import DrlPopPerLayout
    L = _lib()
    for members, cap, mb in ((1, 1, 1), (3, 257, 65), (1024, 100000, 4096)):
        lay, one = DrlPopPerLayout(), DrlPerLayout()
        assert L.drl_pop_per_layout_query(members, cap, mb, ctypes.byref(lay)) == 0, L.drl_last_error()
        assert L.drl_per_layout_query(cap, mb, ctypes.byref(one)) == 0
        for f, _ in DrlPerLayout._fields_:
            assert getattr(lay.member, f) == getattr(one, f), f
        assert lay.member_stride % 16 == 0 and lay.member_stride >= one.bytes
        assert lay.hparams_off % 16 == 0 and lay.hparams_off == lay.member_stride * members
        assert lay.hparams_stride % 16 == 0 and lay.hparams_stride >= 32
        assert lay.bytes == lay.hparams_off + members * lay.hparams_stride
        assert (lay.members, lay.max_batch) == (members, mb)
    assert L.drl_pop_per_layout_query(3, 257, 65, None) != 0 and b"layout is NULL" in L.drl_last_error()


def test_pop_per_layout_header_walk(tmp_path):
    """tests/native/perpop_layout_check.cpp, a stand-alone program under the
    address and undefined-behaviour sanitizers, walks the header the kernels
    share: every byte of every member belongs to exactly one field, the
    records do not overlap the blocks.  Nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "perpop_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "perpop_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_pop_per_calls_validate_before_device_work():
    """Every new call refuses each bad argument by name before any device
    work (no GPU needed): NULL or misaligned pointers, members 0 and 1025,
    capacity 0 and 2^24 + 1, max_batch 0 and 4097, alpha < 0, beta0 > 1,
    beta_steps < 0, eps < 0, size, cursor, count, a conv or f32-obs
    description."""
    from dronerl_amd.dqn import DrlPerHParams, DrlReplay, DrlWidenetDesc, convnet_desc
    from dronerl_amd.population import DrlPopPerLayout
    L = _lib()
    err = L.drl_last_error
    blk, pop = vp(1 << 20), vp(1 << 22)
    lay = DrlPopPerLayout()
    good = (DrlPerHParams * 4)(*[DrlPerHParams(0.6, 0.4, 100, 1e-6)] * 4)
    d = TP._desc()
    D = ctypes.byref(d)
    ring = DrlReplay(1000, 32, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def tree_calls(M, cap, B, b=blk):
        return [L.drl_pop_per_init(M, cap, B, good, b, None), L.drl_pop_per_mark_new(M, cap, B, b, 0, 5, None),
                L.drl_pop_per_rebuild(M, cap, B, b, None)]

    def sample(desc=D, M=4, B=64, p=pop, b=blk, cap=1000, size=100):
        return L.drl_pop_per_sample(desc, M, B, p, b, cap, size, None)

    def train(desc=D, M=4, B=64, p=pop, r=ring, size=100, b=blk):
        return L.drl_pop_per_train(desc, M, B, p, None if r is None else ctypes.byref(r), size, b, None)

    def big_ring(cap):
        return DrlReplay(cap, 32, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    for M, cap, B, word in ((0, 1000, 64, b"members"), (1025, 1000, 64, b"members"), (4, 0, 64, b"capacity"),
                            (4, (1 << 24) + 1, 64, b"capacity"), (4, 1000, 0, b"max_batch"),
                            (4, 1000, 4097, b"max_batch")):
        assert L.drl_pop_per_layout_query(M, cap, B, ctypes.byref(lay)) != 0 and word in err(), word
        for rc in tree_calls(M, cap, B):
            assert rc != 0 and word in err(), (word, err())
        assert sample(M=M, B=B, cap=cap) != 0 and word in err(), (word, err())
        assert train(M=M, B=B, r=big_ring(cap)) != 0 and word in err(), (word, err())
    for rc in tree_calls(4, 1000, 64, None):
        assert rc != 0 and b"prioritized population block" in err()
    for rc in tree_calls(4, 1000, 64, vp((1 << 20) + 8)):
        assert rc != 0 and b"16-byte" in err()
    assert L.drl_pop_per_init(4, 1000, 64, None, blk, None) != 0 and b"hparams are NULL" in err()
    for k, (bad, name) in enumerate(((DrlPerHParams(-0.1, 0.4, 0, 1e-6), b"alpha"),
                                     (DrlPerHParams(float("nan"), 0.4, 0, 1e-6), b"alpha"),
                                     (DrlPerHParams(0.6, 1.5, 0, 1e-6), b"beta0"),
                                     (DrlPerHParams(0.6, -0.1, 0, 1e-6), b"beta0"),
                                     (DrlPerHParams(0.6, 0.4, -1, 1e-6), b"beta_steps"),
                                     (DrlPerHParams(0.6, 0.4, 0, -1e-6), b"eps"))):
        hp = (DrlPerHParams * 4)(*[bad if m == k % 4 else good[0] for m in range(4)])
        assert L.drl_pop_per_init(4, 1000, 64, hp, blk, None) != 0
        assert name in err() and b"member %d" % (k % 4) in err(), (name, err())
    assert L.drl_pop_per_mark_new(4, 1000, 64, blk, -1, 5, None) != 0 and b"cursor" in err()
    assert L.drl_pop_per_mark_new(4, 1000, 64, blk, 1000, 5, None) != 0 and b"cursor" in err()
    assert L.drl_pop_per_mark_new(4, 1000, 64, blk, 0, -1, None) != 0 and b"count" in err()
    # the description: NULL, f32 observation rows, widths, a conv net's description
    conv = ctypes.cast(ctypes.pointer(convnet_desc((7, 7, 6), [dict(out_channels=8, kernel_size=3, padding=1)], (),
                                                   5, "code")), ctypes.POINTER(DrlWidenetDesc))
    for call in (sample, train):
        assert call(desc=None) != 0 and b"NULL" in err()
        assert call(desc=ctypes.byref(TP._desc(294, (64,), inp=0))) != 0 and b"policy code" in err()
        assert call(desc=ctypes.byref(TP._desc(294, (264,)))) != 0 and b"hidden widths" in err()
        assert call(desc=conv) != 0 and err()
        assert call(p=None) != 0 and b"population block" in err()
        assert call(p=vp((1 << 22) + 8)) != 0 and b"16-byte" in err()
        assert call(b=None) != 0 and b"prioritized population block" in err()
        assert call(b=vp((1 << 20) + 4)) != 0 and b"16-byte" in err()
    assert sample(size=0) != 0 and b"size" in err()
    assert sample(size=1001) != 0 and b"size" in err()
    assert train(r=None) != 0 and b"replay" in err()
    assert train(r=DrlReplay(1000, 32, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"NULL" in err()
    assert train(r=DrlReplay(1000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"policy codes" in err()
    assert train(size=-1) != 0 and b"size" in err()
    assert train(size=1001) != 0 and b"size" in err()


def test_per_sweep_cli_grid_and_refusals():
    """per_sweep.parse_args: the four PER options join the grid; each point
    members_seeds times with the right values and seeds; shared options
    inside the grid, conv, widths a population refuses and sharding are
    refused by name; sweep keeps refusing --prioritized_replay as before."""
    from dronerl_amd import per_sweep, sweep
    args, points = per_sweep.parse_args(["--grid", '{"per_alpha": [0, 0.6], "per_beta": [0.4, 1.0]}', "--members_seeds",
                                         "2", "--num_steps", "300", "--seed", "3", "--per_eps", "1e-3"])
    hps, seeds, rows, pers = per_sweep.members_of(args, points)
    assert len(hps) == len(pers) == 8 and seeds == [3, 4] * 4
    assert [(p["alpha"], p["beta0"]) for p in pers] == [(0.0, 0.4)] * 2 + [(0.0, 1.0)] * 2 + [(0.6, 0.4)] * 2 + \
        [(0.6, 1.0)] * 2
    assert all(p["beta_steps"] == 300 and p["eps"] == 1e-3 for p in pers)  # (--per_beta_steps defaults to num_steps)
    assert all(isinstance(p["beta_steps"], int) and isinstance(p["alpha"], float) for p in pers)
    assert [hp.sample_seed for hp in hps] == seeds and rows[3] == {"per_alpha": 0, "per_beta": 1.0, "seed": 4}
    args, points = per_sweep.parse_args(["--grid", '{"per_beta_steps": [0, 50], "per_eps": [1e-6, 0.01], '
                                         '"batch_size": [8, 16]}', "--per_alpha", "0.7", "--prioritized_replay",
                                         "--hidden_layers", "256", "128", "64"])
    hps, seeds, rows, pers = per_sweep.members_of(args, points)
    assert len(pers) == 8 and [hp.batch for hp in hps] == [8, 16] * 4
    assert [(p["beta_steps"], p["eps"]) for p in pers] == [(0, 1e-6)] * 2 + [(0, 0.01)] * 2 + [(50, 1e-6)] * 2 + \
        [(50, 0.01)] * 2
    assert all(p["alpha"] == 0.7 and p["beta0"] == 0.4 for p in pers)
    a3, p3 = per_sweep.parse_args([])
    assert p3 == [{}] and per_sweep.members_of(a3, p3)[3] == [dict(alpha=0.6, beta0=0.4, beta_steps=1000, eps=1e-6)]
    for key, why in (("num_envs", "every member owns num_envs"), ("hidden_layers", "architecture"),
                     ("memory_size", "one allocation"), ("num_steps", "step together"), ("grid_size", "env parameters"),
                     ("seed", "--members_seeds")):
        with pytest.raises(ValueError, match=f"{key} must be shared.*{why}"):
            per_sweep.parse_args(["--grid", json.dumps({key: [1, 2], "per_alpha": [0.5]})])
    with pytest.raises(ValueError, match="not a per-member option"):
        per_sweep.parse_args(["--grid", '{"per_gamma": [1]}'])
    with pytest.raises(ValueError, match="per_alpha must be a non-empty list"):
        per_sweep.parse_args(["--grid", '{"per_alpha": 0.5}'])
    with pytest.raises(ValueError, match="per_beta in"):
        per_sweep.parse_args(["--grid", '{"per_beta": [0.5, 1.5]}'])
    with pytest.raises(ValueError, match="per_alpha and per_eps must be >= 0"):
        per_sweep.parse_args(["--per_alpha", "-1"])
    with pytest.raises(ValueError, match="per_sweep with --network_type conv"):
        per_sweep.parse_args(["--network_type", "conv"])
    with pytest.raises(ValueError, match="per_sweep with --use_sharding"):
        per_sweep.parse_args(["--use_sharding", "--num_envs", "8"])
    for widths in (["264"], ["12"], ["64", "64", "64", "64"]):
        with pytest.raises(ValueError, match="per_sweep: --hidden_layers must be"):
            per_sweep.parse_args(["--hidden_layers", *widths])
    with pytest.raises(ValueError, match="at most 1024"):
        per_sweep.parse_args(["--grid", json.dumps({"per_alpha": [0.5] * 33, "per_eps": [1.0] * 32})])
    with pytest.raises(ValueError, match="--prioritized_replay is not implemented for the population sweep"):
        sweep.parse_args(["--prioritized_replay"])


def test_prioritized_population_python_refusals():
    """train_population(per=...) refuses conv nets by name and a per list of
    the wrong length; a PER record names its bad field (no device)."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.population import per_record, train_population
    with pytest.raises(ValueError, match=r"train_population\(per=...\) with network_type='conv' is not implemented"):
        train_population(EnvParams(), [DQNHParams()], 4, 10, network_type="conv", per=[{}])
    with pytest.raises(ValueError, match="per: one dict of PER hyperparameters per member"):
        train_population(EnvParams(), [DQNHParams()] * 2, 4, 10, per=[{}])
    assert per_record() == dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6)
    for bad, name in ((dict(alpha=-1), "alpha"), (dict(beta0=1.5), "beta0"), (dict(beta_steps=-1), "beta_steps"),
                      (dict(eps=-1), "eps"), (dict(gamma=1), "gamma is not one of")):
        with pytest.raises(ValueError, match=name):
            per_record(bad)


# Every __global__ kernel under csrc/perpop/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_pop_per_init_kernel": "test_population_per.py::test_member_trees_rebuild_to_the_numpy_tree_bit_exact",
    "drl_pop_per_mark_kernel": "test_population_per.py::test_member_trees_rebuild_to_the_numpy_tree_bit_exact",
    "drl_pop_per_rebuild_kernel": "test_population_per.py::test_member_trees_rebuild_to_the_numpy_tree_bit_exact",
    "drl_pop_per_sample_kernel": "test_population_per.py::test_member_samples_are_the_single_agents_bit_exact",
    "drl_pop_per_rows_kernel": "test_population_per.py::test_a_member_is_the_single_agent_bit_exact",
    "drl_pop_per_td_kernel": "test_population_per.py::test_a_member_is_the_single_agent_bit_exact",
    "drl_pop_per_priority_kernel": "test_population_per.py::test_a_member_is_the_single_agent_bit_exact",
}


def test_every_perpop_kernel_has_a_gpu_test():
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "perpop", "*.hip")):
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
def _setup(sizes, hps, pers, E, cap, seed=0, online=None, target=None, max_batch=None):
    """An env of P * E envs (9x9, 4 drones, a 7x7 window), a
    PrioritizedPopulationDQN with random weights and biases, its prioritized
    rings."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.population import PopulationReplay, PrioritizedPopulationDQN, PrioritizedPopulationReplay
    ep = EnvParams(**TP.SHAPES["g9"])
    P = len(hps)
    env = BatchedDeliveryDrones(ep, P * E)
    env.reset(seed=seed)
    if online is None:
        online, target = TP._rand_sets(sizes, P, seed + 11)
    pop = PrioritizedPopulationDQN(sizes[0], sizes[1:-1], hps, E, n_actions=sizes[-1], online=online, target=target,
                                   max_batch=max_batch)
    ppr = PrioritizedPopulationReplay(PopulationReplay(P, cap, ep.window_radius), pers, pop.max_batch)
    return env, pop, ppr, (online, target)


@gpu
@pytest.mark.parametrize("cap", [1, 257, 5000])
def test_member_trees_rebuild_to_the_numpy_tree_bit_exact(cap):
    """3 members.  After drl_pop_per_init every tree is zero and pmax is 1.
    The test writes a different pmax per member, then marks a partly filled
    ring, a range that wraps and count > capacity; after each, every
    member's rebuilt tree equals tests/_per_ref.build_tree of that member's
    leaves, which hold its own pmax.  Capacity 5000 (P = 8192) takes two
    rebuild launches with the member in the grid.  Random leaves over stale
    internal nodes rebuild to the numpy tree too."""
    from dronerl_amd.population import PopulationReplay, PrioritizedPopulationReplay
    M = 3
    ppr = PrioritizedPopulationReplay(PopulationReplay(M, cap, 3), [{}] * M, 8, guard_bytes=4096)
    P = ppr.layout.member.leaves
    assert P == R.leaves_of(cap)
    ppr._alloc[ppr.layout.bytes:].fill_(0xA5)
    records = ppr.block[ppr.layout.hparams_off:].clone()
    torch.cuda.synchronize()
    for m in range(M):
        assert float(ppr.pmax(m).item()) == 1.0 and not ppr.tree(m).any().item()
    want = [np.zeros(P, F) for _ in range(M)]

    def check(where):
        ppr.rebuild()
        torch.cuda.synchronize()
        for m in range(M):
            assert np.array_equal(_bits(_host(ppr.tree(m))), _bits(R.build_tree(want[m]))), (where, m)

    pm = [[3.0, 0.75, 2.5], [0.5, 7.0, 1.25], [1e-3, 1e6, 9.0]]
    n = max(1, cap // 2)  # a partly filled ring
    for m in range(M):
        ppr.pmax(m).fill_(pm[m][0])
        want[m][:n] = pm[m][0]
    ppr._mark(0, n)
    check("partly filled")
    cur, cnt = (cap * 3) // 4, max(1, cap // 2)  # a range that wraps
    for m in range(M):
        ppr.pmax(m).fill_(pm[m][1])
        want[m][(cur + np.arange(cnt)) % cap] = pm[m][1]
    ppr._mark(cur, cnt)
    check("wrapped")
    g = np.random.default_rng(cap)
    for m in range(M):  # random leaves, some zero; stale internal nodes
        want[m][:] = 0
        want[m][:cap] = np.where(g.random(cap) < 0.3, 0.0, g.random(cap) * 10 ** g.uniform(-6, 6, cap)).astype(F)
        ppr.tree(m)[P:].copy_(torch.from_numpy(want[m]))
        if P > 1:
            ppr.tree(m)[1:P].fill_(-1.0)
    check("random")
    check("random, again")
    for m in range(M):  # count > capacity marks every slot (and no pad leaf)
        ppr.pmax(m).fill_(pm[m][2])
        want[m][:] = 0
        want[m][:cap] = pm[m][2]
    ppr._mark(cap // 3, cap + 7)
    check("count > capacity")
    assert torch.equal(ppr.block[ppr.layout.hparams_off:], records)
    assert bool((ppr._alloc[ppr.layout.bytes:] == 0xA5).all())


def _set_step(pop, m, step):
    off = pop.layout.member.counters_off
    pop.member_block(m)[off:off + 4].view(torch.int32).fill_(step)


@gpu
def test_member_samples_are_the_single_agents_bit_exact():
    """3 members with batches 1, 65 and 1030 (a sampler thread's second row)
    at max_batch 1030; capacity 5000 holding 4000 rows; different seeds,
    steps and betas; random positive leaves with 10 % zeros.  Slots, weights
    and wmax of each member equal a solo drl_per_sample on a copy of that
    member's tree with its batch, seed, step and hyperparameters, bit for
    bit; member 1's slots equal tests/_per_ref.sample; the entries behind
    batch_m keep the sentinel."""
    from dronerl_amd.dqn import DQNHParams
    cap, size, batches = 5000, 4000, (1, 65, 1030)
    hps = [DQNHParams(batch=b, sample_seed=s) for b, s in zip(batches, (11, 99, 12345678901))]
    pers = [dict(alpha=0.6, beta0=0.4, beta_steps=10), dict(alpha=1.0, beta0=1.0), dict(alpha=0.3, beta0=0.0, beta_steps=4)]
    steps = (0, 7, 3)
    env, pop, ppr, _ = _setup((294, 16, 5), hps, pers, 2, cap)
    ppr.replay.size = size
    P = ppr.layout.member.leaves
    g = np.random.default_rng(5)
    SLOT, WT = -77, -5.5
    leaves = []
    for m in range(3):
        lv = np.zeros(P, F)
        lv[:size] = np.where(g.random(size) < 0.1, 0.0, g.random(size) * 10 ** g.uniform(-3, 3, size)).astype(F)
        leaves.append(lv)
        ppr.tree(m)[P:].copy_(torch.from_numpy(lv))
        ppr.slots(m).fill_(SLOT)
        ppr.weights(m).fill_(WT)
        _set_step(pop, m, steps[m])
    ppr.rebuild()
    pop.sample(ppr)
    torch.cuda.synchronize()
    for m, b in enumerate(batches):
        solo = TR._per(cap, b, **pers[m])
        solo.tree.copy_(ppr.tree(m))
        solo.sample(hps[m].sample_seed, TR._counters(steps[m]).data_ptr(), size=size)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_host(ppr.tree(m))), _bits(R.build_tree(leaves[m]))), m
        assert torch.equal(ppr.slots(m)[:b], solo.slots), m
        assert torch.equal(ppr.weights(m)[:b].view(torch.int32), solo.weights.view(torch.int32)), m
        assert torch.equal(ppr.wmax(m).view(torch.int32), solo.wmax.view(torch.int32)), m
        assert bool((ppr.slots(m)[b:] == SLOT).all()) and bool((ppr.weights(m)[b:] == WT).all()), m
        s = _host(ppr.slots(m)[:b])
        assert ((s >= 0) & (s < size)).all() and (leaves[m][s] > 0).all() and float(ppr.weights(m)[:b].max()) == 1.0
    assert np.array_equal(_host(ppr.slots(1)[:65]), R.sample(R.build_tree(leaves[1]), 99, 7, 65))


# ---- a member against the single agent ----------------------------------------------------------------------
SOLO_HPS = dict(tau=0.7, target_update_interval=3, epsilon_decay=0.9, epsilon_decay_every=2)
SOLO_MEMBERS = [(8, dict(alpha=0.6, beta0=0.4, beta_steps=6)), (65, dict(alpha=1.0, beta0=1.0)),
                (200, dict(alpha=0.3, beta0=0.0, eps=1e-3)), (64, dict(alpha=0.0, beta0=0.0))]


class _Solo:
    """A PrioritizedDQNLearner + PrioritizedReplay given member m's initial
    parameters and hyperparameters; `follow` copies the member's ring rows
    into its own ring and marks the step's new rows."""

    def __init__(self, sizes, hp, per, cap, online, target):
        from dronerl_amd.dqn import PrioritizedDQNLearner, PrioritizedReplay, QNetwork, ReplayBuffer
        net = QNetwork(sizes[0], sizes[1:-1], n_actions=sizes[-1], precision="f32", input="code")
        net.load(*online)
        self.learner = PrioritizedDQNLearner(net, hp, target=target)
        self.rb = ReplayBuffer(cap, sizes[0], torch.device("cuda"), code_radius=3)
        self.per = PrioritizedReplay(self.rb, batch=hp.batch, **per)

    def follow(self, ring, cursor0, count, cursor, size):
        for k, v in ring.items():
            getattr(self.rb, k).copy_(v)
        self.rb.cursor, self.rb.size = cursor, size
        self.per._mark(cursor0, count)


def _assert_member_is_solo(pop, ppr, m, solo, b, where):
    for k in SETS:
        for l, ((w, bb), (sw, sb)) in enumerate(zip(pop.params(k, m), solo.learner.params(k))):
            assert torch.equal(w.view(torch.int32), sw.view(torch.int32)), (where, m, k, l, "W")
            assert torch.equal(bb.view(torch.int32), sb.view(torch.int32)), (where, m, k, l, "b")
    c, sc = pop.counters(m), solo.learner.counters()
    for k in sc:
        assert np.array([c[k]]).tobytes() == np.array([sc[k]]).tobytes(), (where, m, k, c, sc)
    per = solo.per
    assert torch.equal(ppr.tree(m).view(torch.int32), per.tree.view(torch.int32)), (where, m, "tree")
    assert torch.equal(ppr.pmax(m).view(torch.int32), per.pmax.view(torch.int32)), (where, m, "pmax")
    assert torch.equal(ppr.wmax(m).view(torch.int32), per.wmax.view(torch.int32)), (where, m, "wmax")
    assert torch.equal(ppr.slots(m)[:b], per.slots), (where, m, "slots")
    assert torch.equal(ppr.weights(m)[:b].view(torch.int32), per.weights.view(torch.int32)), (where, m, "weights")
    assert torch.equal(ppr.abs_td(m)[:b].view(torch.int32), per.abs_td.view(torch.int32)), (where, m, "abs_td")


def _run_against_solos(sizes, steps, boost=()):
    """Four members (SOLO_MEMBERS) on rings of 300 slots, 48 rows per step:
    after every step each member equals its solo agent.  Returns, per
    member, the smallest number of duplicate draws over its trained steps."""
    from dronerl_amd.dqn import DQNHParams
    cap, E = 300, 48
    hps = [DQNHParams(batch=b, sample_seed=5 + m, learning_rate=1e-3 * (m + 1), **SOLO_HPS)
           for m, (b, _) in enumerate(SOLO_MEMBERS)]
    pers = [p for _, p in SOLO_MEMBERS]
    env, pop, ppr, (online, target) = _setup(sizes, hps, pers, E, cap, seed=2)
    solos = [_Solo(sizes, hps[m], pers[m], cap, online[m], target[m]) for m in range(4)]
    loop = TP._Loop(env, pop, ppr)
    P = ppr.layout.member.leaves
    dups = [10 ** 9] * 4
    first = []
    for t in range(steps):
        cursor0 = ppr.cursor
        loop.fill()
        for m in range(4):
            solos[m].follow(ppr.ring(m), cursor0, E, ppr.cursor, ppr.size)
            for s in boost:
                ppr.tree(m)[P + s] = 1e6
                solos[m].per.tree[P + s] = 1e6
        trains = [ppr.size >= hp.batch for hp in hps]
        if t == 0:
            first = trains
        if not all(trains):  # a member that has not trained yet: its marked leaves, zero internal nodes
            for m in range(4):
                if not trains[m] and pop.counters(m)["count"] == 0:
                    tree = _host(ppr.tree(m))
                    assert not tree[:P].any() and (tree[P:P + ppr.size] > 0).all(), (t, m)
        pop.train(ppr)
        for m in range(4):
            solos[m].learner.train(solos[m].per)
        torch.cuda.synchronize()
        for m, hp in enumerate(hps):
            _assert_member_is_solo(pop, ppr, m, solos[m], hp.batch, t)
            assert pop.counters(m)["trained"] == int(trains[m]), (t, m)
            if trains[m]:
                s = _host(ppr.slots(m)[:hp.batch])
                dups[m] = min(dups[m], hp.batch - len(set(s.tolist())))
    assert first == [True, False, False, False]  # at step 0 one member trains beside three that do not
    want = [sum(min(E * (t + 1), cap) >= hp.batch for t in range(steps)) for hp in hps]
    assert [pop.counters(m)["count"] for m in range(4)] == want
    assert want == [steps, steps - 1, max(0, steps - 4), steps - 1]
    pop.check_errors()
    return dups


@gpu
@pytest.mark.parametrize("sizes", [(294, 16, 16, 5), (294, 128, 64, 5)], ids=["294-16-16", "294-128-64"])
def test_a_member_is_the_single_agent_bit_exact(sizes):
    """Capacity 300, 48 rows per step into every ring, 12 steps (the ring
    wraps at step 7); members of batch 8 (alpha 0.6, beta0 0.4 over 6
    steps), 65 (alpha 1, beta0 1), 200 (alpha 0.3, beta0 0, eps 1e-3) and 64
    (alpha 0, beta0 0) start training at steps 0, 1, 4 and 1.  Each is
    compared with a solo PrioritizedDQNLearner + PrioritizedReplay given the
    same ring rows, initial parameters and DQNHParams: after every step the
    four parameter sets, the counters, the whole tree, pmax, wmax and the
    step's slots, weights and |td| are equal bit for bit.  A member that has
    not trained yet has its marked leaves and zero internal nodes."""
    _run_against_solos(sizes, 12)


@gpu
def test_member_slots_drawn_twice_take_the_larger_priority():
    """The same on 294-16-16 for 6 steps with leaves 1, 2, 3 and 5 of every
    member raised to 1e6 before every step: in every trained step at least
    batch_m - 4 of a member's rows drew a slot another row drew too (the
    test cannot pass without duplicates), and each member still equals its
    solo agent, whose drawn leaves hold the largest of their rows' new
    priorities."""
    dups = _run_against_solos((294, 16, 16, 5), 6, boost=(1, 2, 3, 5))
    assert all(d >= b - 4 for d, (b, _) in zip(dups, SOLO_MEMBERS)), dups


# ---- a member against the restatement ------------------------------------------------------------------------
def _run_against_restatement(sizes, hps, pers, E, cap, steps, check, ones=()):
    """The loop of test_full_per_matches_the_restatement for the members in
    `check`: after every step tests/_per_ref.per_step, given the device's
    own slots and weights, against the member; its comparison and bounds.
    ones: members whose weights and priorities must be exactly 1.0."""
    env, pop, ppr, _ = _setup(sizes, hps, pers, E, cap, seed=3)
    loop = TP._Loop(env, pop, ppr)
    P = ppr.layout.member.leaves
    sts = {m: TP._state(pop, m) for m in check}
    leaves = {m: np.zeros(P, F) for m in check}
    pmax = {m: F(1.0) for m in check}
    trained = {m: 0 for m in check}
    for t in range(steps):
        cursor = ppr.cursor
        loop.fill()
        size = ppr.size
        rings = {m: {k: _host(v) for k, v in ppr.ring(m).items()} for m in check}
        pop.train(ppr)
        torch.cuda.synchronize()
        for m in check:
            hp, per, r = hps[m], pers[m], rings[m]
            b, seed = hp.batch, hp.sample_seed
            leaves[m][(cursor + np.arange(E)) % cap] = pmax[m]
            ring = (r["obs"], r["next_obs"], r["actions"], r["rewards"], r["dones"])
            tree_dev = _host(ppr.tree(m))
            if size >= b:
                trained[m] += 1
                tree = R.build_tree(leaves[m])
                assert np.array_equal(_bits(tree_dev[1:P]), _bits(tree[1:P])), (t, m)
                slots, w = _host(ppr.slots(m)[:b]), _host(ppr.weights(m)[:b])
                assert np.array_equal(slots, R.sample(tree, seed, t, b)), (t, m)
                w32 = R.weights64(tree, slots, size, R.beta_of(per["beta0"], per.get("beta_steps", 0), t)).astype(F)
                assert (R.ulps(w * F(ppr.wmax(m).item()), w32) <= 4).all(), (t, m)
                if m in ones:
                    assert np.array_equal(_bits(w), _bits(np.ones(b, F))), (t, m)
                info = R.per_step(sts[m], TP._ohp(hp), *ring, size, slots, w, 7)
                TP._assert_member(pop, m, sts[m], t)
                absd = info["absd"]
                assert np.array_equal(_bits(_host(ppr.abs_td(m)[:b])), _bits(absd)), (t, m)
                p_dev = tree_dev[P + slots]
                p_ref = R.priority32(absd, per.get("eps", 1e-6), per["alpha"])
                best = {}
                for s, p in zip(slots.tolist(), p_ref.tolist()):
                    best[s] = max(best.get(s, 0.0), p)
                want = np.array([best[s] for s in slots.tolist()], F)
                assert (R.ulps(p_dev, want) <= 1).all(), (t, m, int((R.ulps(p_dev, want) > 1).sum()))
                if m in ones:
                    assert np.array_equal(_bits(p_dev), _bits(np.ones(b, F))), (t, m)
                leaves[m][slots] = p_dev  # (the device's own leaves from here: a 1-ulp difference must not compound)
                assert np.array_equal(_bits(tree_dev[P:]), _bits(leaves[m])), (t, m)  # no other leaf moved
                pmax[m] = max(pmax[m], F(p_dev.max()))
                assert F(ppr.pmax(m).item()) == pmax[m], (t, m)
            else:
                R.per_step(sts[m], TP._ohp(hp), *ring, size, None, None, 7)
                TP._assert_member(pop, m, sts[m], t)
                assert np.array_equal(_bits(tree_dev[P:]), _bits(leaves[m])), (t, m)
    for m in check:
        assert pop.counters(m)["count"] == trained[m] and trained[m] >= steps - 2, (m, trained)
    pop.check_errors()


@gpu
def test_alpha0_beta0_member_is_the_oracle_bit_exact():
    """One member of three has alpha 0, beta0 0 between two full-PER
    neighbours: its weights and its new priorities are exactly 1.0 and its
    step is oracle/dqn_learner.py's on its drawn rows (_per_ref.per_step with
    weights of 1: the oracle's own pieces), parameters and counters bit for
    bit, for 8 steps on a ring that wraps."""
    from dronerl_amd.dqn import DQNHParams
    hps = [DQNHParams(batch=16, sample_seed=1, **SOLO_HPS), DQNHParams(batch=40, sample_seed=2, **SOLO_HPS),
           DQNHParams(batch=8, sample_seed=3, **SOLO_HPS)]
    pers = [dict(alpha=0.6, beta0=0.4, beta_steps=6), dict(alpha=0.0, beta0=0.0, beta_steps=0), dict(alpha=1.0, beta0=1.0)]
    _run_against_restatement((294, 16, 16, 5), hps, pers, 30, 150, 8, check=(1,), ones=(1,))


@gpu
def test_wide_members_match_the_restatement():
    """Net 294-256-128-64 (no single prioritized agent exists above 128): 2
    members, batch 16 and 64, capacity 200, 40 rows per step, 8 steps.  Each
    member against tests/_per_ref.per_step given the device's own slots and
    weights, with test_full_per_matches_the_restatement's comparison and
    bounds: parameters and counters bit for bit, |d| bit for bit, new leaves
    within 1 f32 ulp of priority32, no other leaf moves, pmax the running
    maximum."""
    from dronerl_amd.dqn import DQNHParams
    hps = [DQNHParams(batch=16, sample_seed=4, **SOLO_HPS), DQNHParams(batch=64, sample_seed=5, learning_rate=3e-3, **SOLO_HPS)]
    pers = [dict(alpha=0.6, beta0=0.4, beta_steps=6), dict(alpha=0.8, beta0=0.5, beta_steps=0, eps=1e-3)]
    _run_against_restatement((294, 256, 128, 64, 5), hps, pers, 40, 200, 8, check=(0, 1))


@gpu
def test_prioritized_members_do_not_depend_on_each_other():
    """Member m of a mixed population of 5 equals a population of one with
    env_offset + m E, the same record and seed, after 10 steps of
    train_population(per=...) on a 9x9 grid with 4 drones and 8 envs per
    member (a ring of 60 slots: it wraps): parameters, counters, tree, pmax
    and ring, bit for bit."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.population import PrioritizedPopulationDQN, PrioritizedPopulationReplay, train_population
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)
    E, steps, cap, off = 8, 10, 60, 16
    hps = [DQNHParams(batch=b, num_steps=steps, sample_seed=10 + m, learning_rate=1e-3 * (m + 1), target_update_interval=2 + m % 2)
           for m, b in enumerate((4, 16, 40, 8, 24))]
    pers = [dict(alpha=0.6, beta0=0.4, beta_steps=10), dict(alpha=0.0, beta0=0.0), dict(alpha=1.0, beta0=1.0, eps=1e-2),
            dict(alpha=0.4, beta0=0.7, beta_steps=5), dict(alpha=0.8, beta0=0.0)]
    seeds = [3, 1, 4, 1, 5]
    kw = dict(hidden=(16, 16), reset_env_every=4, memory_size=cap, seed=2)
    full = train_population(ep, hps, E, steps, env_offset=off, seeds=seeds, per=pers, **kw)
    assert isinstance(full.pop, PrioritizedPopulationDQN) and isinstance(full.replay, PrioritizedPopulationReplay)
    assert [full.pop.counters(m)["count"] for m in range(5)] == [10, 9, 6, 10, 8]
    for m in range(5):
        one = train_population(ep, [hps[m]], E, steps, env_offset=off + m * E, seeds=[seeds[m]], per=[pers[m]],
                               max_batch=full.pop.max_batch, **kw)
        for k in SETS:
            for (w, b), (w1, b1) in zip(full.pop.params(k, m), one.pop.params(k, 0)):
                assert torch.equal(w.view(torch.int32), w1.view(torch.int32)), (m, k)
                assert torch.equal(b.view(torch.int32), b1.view(torch.int32)), (m, k)
        assert full.pop.counters(m) == one.pop.counters(0), m
        assert torch.equal(full.replay.member_block(m), one.replay.member_block(0)), m  # tree, pmax, wmax, the draw
        assert float(full.replay.tree(m)[1].item()) > 0
        for k, v in full.replay.ring(m).items():
            assert torch.equal(v, one.replay.ring(0)[k]), (m, k)


@gpu
def test_prioritized_pop_step_replays_from_a_captured_graph():
    """One captured step -- act, the env step with its code, the add and its
    mark, drl_pop_per_train -- replayed 5 times equals 5 eager steps on a
    twin: the parameter sets, the counters and the whole prioritized block.
    3 members with batches 3, 12 and 40.  A capture freezes the host's part
    of a step, the ring's cursor and size among them (both are call
    arguments), so whether a member trains cannot change between replays:
    the batch-40 member holds less than a batch in every replay and only
    blends its target, decays epsilon and advances its step, beside two
    members that train."""
    from dronerl_amd.dqn import DQNHParams
    sizes, E, cap, k = (294, 32, 16, 5), 4, 64, 5
    hps = [DQNHParams(batch=3, sample_seed=1, epsilon_decay=0.9, epsilon_decay_every=1),
           DQNHParams(batch=12, sample_seed=2, tau=0.5, target_update_interval=2, learning_rate=3e-3),
           DQNHParams(batch=40, sample_seed=3, tau=0.5, target_update_interval=1)]
    pers = [dict(alpha=0.6, beta0=0.4, beta_steps=4), dict(alpha=1.0, beta0=1.0), dict(alpha=0.5, beta0=0.5)]
    online, target = TP._rand_sets(sizes, 3, 31)

    def fresh():
        env, pop, ppr, _ = _setup(sizes, hps, pers, E, cap, seed=6, online=online, target=target)
        env.refill_every = 0  # (where the respawn draws happen, never what they are)
        loop = TP._Loop(env, pop, ppr)
        for _ in range(4):
            loop.fill()
        rew = torch.empty((3 * E, 4), dtype=torch.float32, device="cuda")
        don = torch.empty((3 * E, 4), dtype=torch.uint8, device="cuda")
        c0, s0 = ppr.cursor, ppr.size

        def step():
            pop.act(loop.cur, 9, seed=3, actions=loop.acts, synth=(5, 9))
            env.step(loop.acts, rewards=rew, dones=don, code=loop.nxt)
            ppr.replay.cursor, ppr.replay.size = c0, s0
            ppr.add(loop.cur, loop.acts, rew, loop.nxt, don)
            pop.train(ppr)
            loop.cur.copy_(loop.nxt)
        return env, pop, ppr, step

    env, pop, ppr, step = fresh()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    env2, pop2, ppr2, step2 = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step2()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert pop2.counters(0)["step"] == 0  # (capturing runs nothing)
    for _ in range(k):
        g.replay()
    torch.cuda.synchronize()
    env2.check_errors()
    for m in range(3):
        for key in SETS:
            for (w, b), (w2, b2) in zip(pop.params(key, m), pop2.params(key, m)):
                assert torch.equal(w.view(torch.int32), w2.view(torch.int32)), (m, key)
                assert torch.equal(b.view(torch.int32), b2.view(torch.int32)), (m, key)
        assert pop.counters(m) == pop2.counters(m), m
    assert torch.equal(ppr.block, ppr2.block)
    assert [pop2.counters(m)["count"] for m in range(3)] == [k, k, 0] and pop2.counters(2)["step"] == k
    assert float(ppr2.pmax(2).item()) == 1.0 and not ppr2.tree(2)[:ppr2.layout.member.leaves].any().item()
    assert float(ppr2.tree(0)[1].item()) > 0


@gpu
def test_per_sweep_cli_end_to_end(tmp_path):
    """`python -m dronerl_amd.per_sweep --grid '{"per_alpha": [0, 0.6]}'
    --members_seeds 2` at test_sweep_cli_end_to_end's sizes: a table of 4
    rows with the four PER columns and finite eval means."""
    from dronerl_amd import per_sweep
    out = per_sweep.main(["--grid", '{"per_alpha": [0, 0.6]}', "--members_seeds", "2", "--num_envs", "4", "--num_steps",
                          "40", "--num_evals", "2", "--num_eval_steps", "50", "--hidden_layers", "16", "16",
                          "--output_dir", str(tmp_path)])
    table = json.load(open(out["table_path"]))["table"]
    assert len(table) == 4 and out["members"] == 4
    assert [(r["per_alpha"], r["seed"]) for r in table] == [(0.0, 0), (0.0, 1), (0.6, 0), (0.6, 1)]
    for r in table:
        assert (r["per_beta"], r["per_beta_steps"], r["per_eps"]) == (0.4, 40, 1e-6)
        assert r["steps"] == 40 and r["train_steps"] == 40 - (r["batch_size"] // 4 - 1)
        assert np.isfinite([r["eval_reward_mean"], r["eval_reward_std"], r["final_loss"]]).all()
        assert r["pmax"] >= 1.0
