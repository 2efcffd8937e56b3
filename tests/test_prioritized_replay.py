"""Prioritized experience replay on the device (Schaul et al. 2016, the
proportional variant): drl_per_* and drl_dqn_per_train
(dronerl_amd/csrc/per/), dqn.PrioritizedReplay, dqn.PrioritizedDQNLearner,
dqn.make_learner(per=True) and `python -m dronerl_amd.train
--prioritized_replay`.

The reference samples uniformly (jax_impl/buffers.py:79-90); this option has
no counterpart there.  What pins it:
  * tests/_per_ref.py, a numpy restatement of the tree (node = left + right,
    one f32 addition), the stratified descent and the float64 formulas;
  * oracle/dqn_learner.py: with alpha = 0 and beta = 0 every weight and
    priority is exactly 1.0 and a step must be the oracle's learner_step on
    the drawn rows BIT FOR BIT; with priorities on, _per_ref.per_step (the
    oracle's pieces with the weight on the squared error and the delta)
    given the device's own slots and weights of that step.
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

from oracle import dqn_learner as O
from tests import _per_ref as R

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SETS = ("online", "target", "m", "v")
F = np.float32
vp = ctypes.c_void_p


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind
    return _bind(lib())


def _desc(in_features, hidden, inp=0, precision=1, n_actions=5):
    from dronerl_amd.dqn import DrlQnetDesc
    h = list(hidden) + [0] * (3 - len(hidden))
    return DrlQnetDesc(in_features, len(hidden), (ctypes.c_int32 * 3)(*h), n_actions, precision, inp)


# ------------------------------------------------------------------- CPU ---
def test_per_layout_query():
    """Host only: P, the offsets (disjoint, 16-byte aligned, in the header's
    order), the refusals by name."""
    from dronerl_amd.dqn import DrlPerLayout
    L = _lib()
    for cap, P in ((1, 1), (2, 2), (255, 256), (256, 256), (257, 512), (100_000, 131072), (1 << 24, 1 << 24)):
        for batch in (1, 65, 4096):
            lay = DrlPerLayout()
            assert L.drl_per_layout_query(cap, batch, ctypes.byref(lay)) == 0, L.drl_last_error()
            assert (lay.capacity, lay.leaves, lay.batch) == (cap, P, batch)
            marks = [lay.tree_off, lay.pmax_off, lay.wmax_off, lay.slots_off, lay.weights_off, lay.absd_off, lay.bytes]
            need = [8 * P, 4, 4, 8 * batch, 4 * batch, 4 * batch]
            assert marks[0] == 0 and all(m % 16 == 0 for m in marks)
            assert all(marks[i] + need[i] <= marks[i + 1] for i in range(6))
    lay = DrlPerLayout()
    for cap in (0, -1, (1 << 24) + 1):
        assert L.drl_per_layout_query(cap, 8, ctypes.byref(lay)) != 0
        assert b"capacity must be in [1, 2^24]" in L.drl_last_error()
    for batch in (0, 4097, -3):
        assert L.drl_per_layout_query(100, batch, ctypes.byref(lay)) != 0
        assert b"batch must be in [1, 4096]" in L.drl_last_error()
    assert L.drl_per_layout_query(100, 8, None) != 0 and b"layout is NULL" in L.drl_last_error()


def test_per_layout_header_walk(tmp_path):
    """tests/native/per_layout_check.cpp, a stand-alone program under the
    address and undefined-behaviour sanitizers, walks the header the kernels
    share: the block's regions, and the rebuild's launches run on a host
    tree (every internal node written once, from nodes already final, equal
    to the bottom-up tree bit for bit).  Nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "per_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "per_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_per_calls_validate_before_device_work():
    """Every call refuses bad arguments by name before any device work (no
    GPU needed): NULL or misaligned pointers, capacity, batch, size, cursor,
    count, alpha, beta0, beta_steps, eps."""
    from dronerl_amd.dqn import DQNHParams, DrlPerHParams, DrlReplay
    L = _lib()
    blk, ctr = vp(1 << 20), vp(1 << 22)
    err = lambda: L.drl_last_error()  # noqa: E731
    for f, extra in ((L.drl_per_init, ()), (L.drl_per_rebuild, ()), (L.drl_per_mark_new, (0, 5))):
        assert f(1000, 64, None, *extra, None) != 0 and b"prioritized replay block" in err()
        assert f(1000, 64, vp((1 << 20) + 8), *extra, None) != 0 and b"16-byte" in err()
        assert f(0, 64, blk, *extra, None) != 0 and b"capacity" in err()
        assert f((1 << 24) + 1, 64, blk, *extra, None) != 0 and b"capacity" in err()
        assert f(1000, 0, blk, *extra, None) != 0 and b"batch" in err()
        assert f(1000, 4097, blk, *extra, None) != 0 and b"batch" in err()
    assert L.drl_per_mark_new(1000, 64, blk, -1, 5, None) != 0 and b"cursor" in err()
    assert L.drl_per_mark_new(1000, 64, blk, 1000, 5, None) != 0 and b"cursor" in err()
    assert L.drl_per_mark_new(1000, 64, blk, 0, -1, None) != 0 and b"count" in err()
    good = DrlPerHParams(0.6, 0.4, 100, 1e-6)
    bad_hp = ((DrlPerHParams(-0.1, 0.4, 0, 1e-6), b"alpha"), (DrlPerHParams(float("nan"), 0.4, 0, 1e-6), b"alpha"),
              (DrlPerHParams(0.6, -0.1, 0, 1e-6), b"beta0"), (DrlPerHParams(0.6, 1.5, 0, 1e-6), b"beta0"),
              (DrlPerHParams(0.6, 0.4, -1, 1e-6), b"beta_steps"), (DrlPerHParams(0.6, 0.4, 0, -1e-6), b"eps"))

    def sample(cap=1000, batch=64, b=blk, h=good, c=ctr, size=100):
        return L.drl_per_sample(cap, batch, b, None if h is None else ctypes.byref(h), 7, c, size, None)
    assert sample(b=None) != 0 and b"prioritized replay block" in err()
    assert sample(cap=0) != 0 and b"capacity" in err()
    assert sample(batch=4097) != 0 and b"batch" in err()
    assert sample(h=None) != 0 and b"hparams are NULL" in err()
    for h, name in bad_hp:
        assert sample(h=h) != 0 and name in err(), name
    assert sample(c=None) != 0 and b"d_counters" in err()
    assert sample(c=vp((1 << 22) + 4)) != 0 and b"d_counters" in err()
    assert sample(size=0) != 0 and b"size" in err()
    assert sample(size=1001) != 0 and b"size" in err()

    d, dc = _desc(294, (128, 64)), _desc(294, (128, 64), 1)
    hp = DQNHParams(batch=1024).c()
    ring = DrlReplay(5000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def train(desc=d, h=hp, ph=good, agent=vp(1 << 20), packed=vp(1 << 21), r=ring, size=100, per=vp(1 << 23)):
        return L.drl_dqn_per_train(ctypes.byref(desc), None if h is None else ctypes.byref(h),
                                   None if ph is None else ctypes.byref(ph), agent, packed,
                                   None if r is None else ctypes.byref(r), size, per, None)
    assert train(h=None) != 0 and b"hparams is NULL" in err()
    assert train(ph=None) != 0 and b"hparams are NULL" in err()
    for h, name in bad_hp:
        assert train(ph=h) != 0 and name in err(), name
    assert train(agent=None) != 0 and b"agent block" in err()
    assert train(agent=vp((1 << 20) + 8)) != 0 and b"16-byte" in err()
    assert train(packed=None) != 0 and b"packed" in err()
    assert train(r=None) != 0 and b"replay" in err()
    assert train(per=None) != 0 and b"prioritized replay block" in err()
    assert train(per=vp((1 << 23) + 4)) != 0 and b"16-byte" in err()
    assert train(size=-1) != 0 and b"size" in err()
    assert train(size=5001) != 0 and b"size" in err()
    big = DrlReplay((1 << 24) + 1, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    assert train(r=big) != 0 and b"capacity must be in [1, 2^24]" in err()
    assert train(desc=dc) != 0 and b"policy code" in err()  # f32 rows for a code net
    for batch in (0, 4097):
        assert train(h=DQNHParams(batch=batch).c()) != 0 and b"batch" in err()
    assert train(desc=_desc(294, (136,))) != 0 and b"hidden widths" in err()
    assert train(h=DQNHParams(batch=100, target_update_interval=0).c()) != 0 and b"target_update_interval" in err()


def test_per_options_routing_and_cli_refusals(monkeypatch):
    """--prioritized_replay parses into PrioritizedReplay's keywords
    (--per_beta_steps defaults to num_steps); make_learner(per=True) routes
    to PrioritizedDQNLearner at every batch (the classes stubbed: no device)
    and refuses conv and wide nets; the CLI refuses conv, wide and sharded
    runs and the sweep, league and self-play drivers by name."""
    from dronerl_amd import dqn, league, selfplay, sweep
    from dronerl_amd.train import parse_args, per_options_of
    a = parse_args(["--prioritized_replay", "--num_steps", "500"])
    assert per_options_of(a) == dict(alpha=0.6, beta0=0.4, beta_steps=500, eps=1e-6)
    a = parse_args(["--prioritized_replay", "--per_alpha", "0.5", "--per_beta", "0.7", "--per_beta_steps", "0",
                    "--per_eps", "1e-3"])
    assert per_options_of(a) == dict(alpha=0.5, beta0=0.7, beta_steps=0, eps=1e-3)
    assert per_options_of(parse_args([])) is None
    made = []
    for name in ("DQNLearner", "LargeBatchDQNLearner", "PrioritizedDQNLearner"):
        monkeypatch.setattr(dqn, name, lambda net, hp, _n=name, **kw: made.append((_n, hp.batch, kw)) or _n)
    for batch in (1, 8, 64, 65, 4096):
        assert dqn.make_learner(object(), dqn.DQNHParams(batch=batch), per=True, generator=None) == \
            "PrioritizedDQNLearner"
        assert made[-1] == ("PrioritizedDQNLearner", batch, {"generator": None})
    assert dqn.make_learner(object(), dqn.DQNHParams(batch=8)) == "DQNLearner"
    assert dqn.make_learner(object(), dqn.DQNHParams(batch=65), per=False) == "LargeBatchDQNLearner"
    for cls in (dqn.WideQNetwork, dqn.ConvQNetwork):
        with pytest.raises(ValueError, match="prioritized replay trains dense nets of hidden widths up to 128"):
            dqn.make_learner(cls.__new__(cls), dqn.DQNHParams(), per=True)
    with pytest.raises(ValueError, match="--prioritized_replay with --network_type conv"):
        parse_args(["--prioritized_replay", "--network_type", "conv"])
    with pytest.raises(ValueError, match="--prioritized_replay with --hidden_layers wider than 128"):
        parse_args(["--prioritized_replay", "--hidden_layers", "256", "128", "64"])
    with pytest.raises(ValueError, match="--prioritized_replay with --use_sharding"):
        parse_args(["--prioritized_replay", "--use_sharding", "--num_envs", "8"])
    with pytest.raises(ValueError, match="per_beta"):
        parse_args(["--prioritized_replay", "--per_beta", "1.5"])
    for mod, name in ((sweep, "the population sweep"), (league, "the league"), (selfplay, "self-play")):
        with pytest.raises(ValueError, match=f"--prioritized_replay is not implemented for {name}"):
            mod.parse_args(["--prioritized_replay"])
    for v in (dict(alpha=-1.0), dict(beta0=2.0), dict(beta_steps=-1), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            dqn.PrioritizedReplay(object.__new__(dqn.ReplayBuffer), **v)
    with pytest.raises(ValueError, match="wraps a dqn.ReplayBuffer"):
        dqn.PrioritizedReplay(object())


def test_restated_sampler_never_lands_on_an_empty_slot():
    """tests/_per_ref.py's descent (the rule the kernel is checked against):
    on partly filled rings, priorities of 1e-30 beside 1e19 and all-equal
    priorities every drawn slot has a positive leaf; priorities 1:2:3:4 are
    drawn in those proportions."""
    g = np.random.default_rng(3)
    for cap in (1, 2, 3, 255, 256, 257, 5000):
        P = R.leaves_of(cap)
        for kind in ("equal", "extreme", "sparse"):
            leaves = np.zeros(P, F)
            n = max(1, cap // 2) if kind == "sparse" else cap
            if kind == "equal":
                leaves[:n] = F(0.3)
            elif kind == "extreme":
                leaves[:n] = F(1e-30)
                leaves[g.integers(0, n)] = F(1e19)
            else:
                leaves[:n] = np.where(g.random(n) < 0.5, g.random(n), 0).astype(F)
                leaves[g.integers(0, n)] = F(0.5)
            tree = R.build_tree(leaves)
            for B in (1, 3, 64):
                for step in range(3):
                    s = R.sample(tree, 11, step, B)
                    assert ((s >= 0) & (s < n)).all() and (leaves[s] > 0).all(), (cap, kind, B)
    tree = R.build_tree(np.array([1, 2, 3, 4], F))
    counts = np.zeros(4)
    for step in range(32):
        counts += np.bincount(R.sample(tree, 5, step, 4000), minlength=4)
    assert np.abs(counts / counts.sum() - np.array([0.1, 0.2, 0.3, 0.4])).max() < 2e-3


# Every __global__ kernel under csrc/per/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_per_init_kernel": "test_prioritized_replay.py::test_tree_rebuild_is_the_numpy_tree_bit_exact",
    "drl_per_mark_kernel": "test_prioritized_replay.py::test_tree_rebuild_is_the_numpy_tree_bit_exact",
    "drl_per_rebuild_kernel": "test_prioritized_replay.py::test_tree_rebuild_is_the_numpy_tree_bit_exact",
    "drl_per_sample_kernel": "test_prioritized_replay.py::test_sample_is_the_stated_descent_and_weights_within_one_ulp",
    "drl_dqn_per_rows_kernel": "test_prioritized_replay.py::test_alpha0_beta0_is_the_oracle_bit_exact",
    "drl_dqn_per_td_kernel": "test_prioritized_replay.py::test_full_per_matches_the_restatement",
    "drl_dqn_per_priority_kernel": "test_prioritized_replay.py::test_full_per_matches_the_restatement",
    # (every oracle case starts with a ring smaller than the batch: the target blend alone, when due)
}


def test_every_per_kernel_has_a_gpu_test():
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "per", "*.hip")):
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
    return np.ascontiguousarray(a, F).view(np.uint32)


def _per(cap, batch, **kw):
    """A PrioritizedReplay over a small f32 ring (its rows are not read)."""
    from dronerl_amd.dqn import PrioritizedReplay, ReplayBuffer
    return PrioritizedReplay(ReplayBuffer(cap, 4, torch.device("cuda")), batch=batch, **kw)


def _counters(step):
    """A drl_dqn_counters on the device holding `step`."""
    c = torch.zeros(16, dtype=torch.int32, device="cuda")
    c[0] = step
    return c


@gpu
@pytest.mark.parametrize("cap", [1, 2, 255, 256, 257, 5000])
def test_tree_rebuild_is_the_numpy_tree_bit_exact(cap):
    """drl_per_init zeroes the tree and sets pmax = 1; mark_new over a range
    that wraps, over a partly filled ring and with count > capacity sets
    exactly those leaves to pmax; random leaves uploaded by the test (some
    zero, pad leaves zero) rebuild to the numpy tree bit for bit -- one
    launch up to 4096 leaves, two at 5000 (P = 8192) -- and a second rebuild
    over stale internal nodes gives the same tree."""
    per = _per(cap, 8)
    P = per.layout.leaves
    assert P == R.leaves_of(cap) and per.tree.numel() == 2 * P
    torch.cuda.synchronize()
    assert float(per.pmax.item()) == 1.0 and not per.tree.any().item()
    g = np.random.default_rng(cap)
    # a partly filled ring: the first half marked, at pmax = 3
    per.pmax.fill_(3.0)
    n = max(1, cap // 2)
    per._mark(0, n)
    want = np.zeros(P, F)
    want[:n] = 3.0
    per.rebuild()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_host(per.tree)), _bits(R.build_tree(want)))
    # a range that wraps, at another pmax
    per.pmax.fill_(0.75)
    cur, cnt = (cap * 3) // 4, max(1, cap // 2)
    per._mark(cur, cnt)
    want[(cur + np.arange(cnt)) % cap] = 0.75
    per.rebuild()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_host(per.tree)), _bits(R.build_tree(want)))
    # random leaves, some of them zero; stale internal nodes
    leaves = np.zeros(P, F)
    leaves[:cap] = np.where(g.random(cap) < 0.3, 0.0, g.random(cap) * 10 ** g.uniform(-6, 6, cap)).astype(F)
    per.tree[P:].copy_(torch.from_numpy(leaves))
    if P > 1:
        per.tree[1:P].fill_(-1.0)
    for _ in range(2):
        per.rebuild()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_host(per.tree)), _bits(R.build_tree(leaves)))
    # count > capacity marks every slot (and no pad leaf)
    per.pmax.fill_(2.5)
    per._mark(cap // 3, cap + 7)
    per.rebuild()
    torch.cuda.synchronize()
    full = np.zeros(P, F)
    full[:cap] = 2.5
    assert np.array_equal(_bits(_host(per.tree)), _bits(R.build_tree(full)))


def _leaves_of_kind(kind, cap, P, g):
    """(leaves f32 [P], size): the trees the sampler is checked on."""
    leaves = np.zeros(P, F)
    size = cap
    if kind == "random":
        leaves[:cap] = (g.random(cap) * 10 ** g.uniform(-3, 3, cap)).astype(F)
    elif kind == "equal":
        leaves[:cap] = F(0.6)
    elif kind == "many-zero":
        size = max(1, (cap * 2) // 3)  # a partly filled ring, most of its slots at priority 0
        leaves[:size] = np.where(g.random(size) < 0.9, 0.0, g.random(size)).astype(F)
        leaves[size - 1] = F(0.25)
    elif kind == "extreme":
        leaves[:cap] = F(1e-30)
        leaves[cap // 2] = F(1e19)
    else:  # "size-1": one slot written
        size = 1
        leaves[0] = F(1.0)
    return leaves, size


ULP_STATS = {}


@gpu
@pytest.mark.parametrize("kind", ["random", "equal", "many-zero", "extreme", "size-1"])
def test_sample_is_the_stated_descent_and_weights_within_one_ulp(kind):
    """drl_per_sample on a rebuilt tree, capacities 255 (the whole tree in
    LDS) and 5000 (the top in LDS, the rest from L2), batches 1, 3, 64, 1000
    and 4096, two steps each, beta annealed: the slots equal the header's
    pseudocode (tests/_per_ref.sample) exactly, every slot is < size with a
    positive leaf.

    The weights: the device rounds pow(size * leaf / root, -beta), a double
    pow accurate to under one double ulp, once to f32, and so does numpy; two
    such roundings of values under a double ulp apart differ by at most 1
    f32 ulp (derived, not measured), so every weight must be f32(c / wmax)
    for a c within 1 ulp of numpy's w, wmax itself within 1 ulp of numpy's
    largest w, and the largest weight exactly 1.0 (w / wmax is one f32
    division of the device's own values).  The share of weights that differ
    from f32(numpy's w / the device's wmax) goes to profiles/per/ulp.json."""
    g = np.random.default_rng(17)
    beta0, beta_steps, seed = 0.4, 10, 99
    differ = total = 0
    for cap in (255, 5000):
        for B in (1, 3, 64, 1000, 4096):
            per = _per(cap, B, alpha=0.6, beta0=beta0, beta_steps=beta_steps)
            P = per.layout.leaves
            leaves, size = _leaves_of_kind(kind, cap, P, g)
            per.tree[P:].copy_(torch.from_numpy(leaves))
            per.rebuild()
            tree = R.build_tree(leaves)
            for step in (0, 7):
                ctr = _counters(step)
                per.sample(seed, ctr.data_ptr(), size=size)
                torch.cuda.synchronize()
                slots, w, wmax = _host(per.slots), _host(per.weights), F(per.wmax.item())
                want = R.sample(tree, seed, step, B)
                assert np.array_equal(slots, want), (cap, B, step)
                assert ((slots >= 0) & (slots < size)).all() and (leaves[slots] > 0).all()
                w64 = R.weights64(tree, want, size, R.beta_of(beta0, beta_steps, step))
                w32 = w64.astype(F)
                assert R.ulps(np.array([wmax]), np.array([w32.max()]))[0] <= 1, (cap, B, step, wmax, w32.max())
                cands = [(c / wmax).astype(F) for c in (w32, np.nextafter(w32, F(np.inf)), np.nextafter(w32, F(0)))]
                ok = (w == cands[0]) | (w == cands[1]) | (w == cands[2])
                assert ok.all(), (cap, B, step, int((~ok).sum()))
                assert w.max() == F(1.0) and (w > 0).all()
                differ += int((_bits(w) != _bits(cands[0])).sum())
                total += B
    ULP_STATS[kind] = {"weights": total, "not_identical": differ, "share": differ / total}
    if len(ULP_STATS) < 5:  # (the record is written once every tree has run)
        return
    try:
        os.makedirs(os.path.join(REPO, "profiles", "per"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "per", "ulp.json"), "w") as f:
            json.dump({"what": "share of drl_per_sample weights not bit-identical to f32(numpy float64 w / device "
                               "wmax); every one is within 1 f32 ulp of w (asserted)",
                       "trees": dict(sorted(ULP_STATS.items()))}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


# ---- the learner -------------------------------------------------------------------------------------------
def _net_and_target(sizes, inp, seed, n_actions=5):
    from dronerl_amd.dqn import QNetwork
    g = torch.Generator().manual_seed(seed + 5)
    net = QNetwork(sizes[0], sizes[1:-1], n_actions=n_actions, generator=g, precision="f32", input=inp)
    gb = torch.Generator(device="cuda").manual_seed(seed + 6)
    for b in net.biases:
        b.normal_(0, 0.05, generator=gb)
    net.pack()
    target = ([torch.randn(w.shape, generator=g) * 0.1 for w in net.weights],
              [torch.randn(b.shape, generator=g) * 0.05 for b in net.biases])
    return net, target


def _setup(sizes, inp, hp_kw, E, cap, per_kw, seed=0):
    """An env whose window gives sizes[0] inputs, a net with random biases, a
    PrioritizedDQNLearner with its own target, a prioritized ring."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams, PrioritizedDQNLearner, PrioritizedReplay, ReplayBuffer, make_learner
    radius = {150: 2, 294: 3}[sizes[0]]
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=radius), E)
    env.reset(seed=seed)
    net, target = _net_and_target(sizes, inp, seed)
    hp = DQNHParams(**hp_kw)
    learner = make_learner(net, hp, per=True, target=target)
    assert isinstance(learner, PrioritizedDQNLearner)
    rb = ReplayBuffer(cap, sizes[0], torch.device("cuda"), code_radius=radius if inp == "code" else 0)
    return env, net, learner, PrioritizedReplay(rb, **per_kw), hp


class _Loop:
    """train_jax.py's loop shape around a learner: act with the device
    epsilon, step, add_many into the prioritized ring (the caller trains)."""

    def __init__(self, env, net, learner, per, inp):
        self.env, self.net, self.learner, self.per, self.inp = env, net, learner, per, inp
        E, W = env.num_envs, 2 * env.params.window_radius + 1
        new = env.new_code if inp == "code" else (lambda: torch.empty((E, 1, W, W, 6), device="cuda"))
        self.cur, self.nxt = new(), new()
        if inp == "code":
            env.get_code(out=self.cur)
        else:
            env.get_obs(1, out=self.cur)
        self.acts = torch.empty((E, 8), dtype=torch.int32, device="cuda")
        self.t = 0

    def fill(self):
        E = self.env.num_envs
        x = self.cur if self.inp == "code" else self.cur.reshape(E, -1)
        self.net.act(x, self.learner.epsilon, seed=3, step=self.t, actions=self.acts, synth=(5, self.t))
        if self.inp == "code":
            r, d = self.env.step(self.acts, code=self.nxt)
        else:
            r, d, _ = self.env.step(self.acts, obs_k=1, obs=self.nxt)
        self.per.add_many(self.cur, self.acts, r, self.nxt, d)
        self.cur, self.nxt = self.nxt, self.cur
        self.t += 1


def _state(learner):
    st = O.LearnerState.start([(_host(w), _host(b)) for w, b in learner.params("online")],
                              [(_host(w), _host(b)) for w, b in learner.params("target")], 1.0)
    st.m = [(_host(w), _host(b)) for w, b in learner.params("m")]
    st.v = [(_host(w), _host(b)) for w, b in learner.params("v")]
    c = learner.counters()
    st.step, st.count, st.epsilon = c["step"], c["count"], np.float32(c["epsilon"])
    st.beta1_pow, st.beta2_pow = c["beta1_pow"], c["beta2_pow"]
    return st


def _ohp(hp):
    return O.HParams(batch=hp.batch, gamma=hp.gamma, learning_rate=hp.learning_rate, beta1=hp.beta1, beta2=hp.beta2,
                     adam_eps=hp.adam_eps, tau=hp.tau, target_update_interval=hp.target_update_interval,
                     epsilon_decay=hp.decay(), epsilon_end=hp.epsilon_end,
                     epsilon_decay_every=hp.epsilon_decay_every, sample_seed=hp.sample_seed)


def _ring(rb):
    return _host(rb.obs), _host(rb.next_obs), _host(rb.actions), _host(rb.rewards), _host(rb.dones)


def _assert_same(learner, st, where):
    for k in SETS:
        for l, ((w, b), (ow, ob)) in enumerate(zip(learner.params(k), getattr(st, k))):
            assert np.array_equal(_bits(_host(w)), _bits(ow)), (where, k, l, "W")
            assert np.array_equal(_bits(_host(b)), _bits(ob)), (where, k, l, "b")
    c = learner.counters()
    assert c["step"] == st.step and c["count"] == st.count, where
    assert np.float32(c["epsilon"]) == st.epsilon and np.float32(c["loss"]) == st.loss, where
    assert c["beta1_pow"] == st.beta1_pow and c["beta2_pow"] == st.beta2_pow, where


# net, batch -> envs per step, ring capacity (the ring wraps within the 10 steps; the first steps hold less than
# a batch, and every case takes one step on the empty ring)
ORACLE_NETS = {"16-16-w5": (150, 16, 16, 5), "128-64-w7": (294, 128, 64, 5)}
ORACLE_BATCHES = {1: (24, 100), 8: (5, 30), 65: (30, 200), 1000: (400, 2500)}


@gpu
@pytest.mark.parametrize("inp", ["code", "obs"])
@pytest.mark.parametrize("batch", [1, 8, 65, 1000])
@pytest.mark.parametrize("net_id", list(ORACLE_NETS))
def test_alpha0_beta0_is_the_oracle_bit_exact(net_id, batch, inp, monkeypatch):
    """alpha = 0 and beta = 0: pow(x, +-0) is exactly 1, so every weight and
    every priority is 1.0 and a step is oracle/dqn_learner.py's learner_step
    on the rows sample_slots names: all four parameter sets, the loss, every
    counter and both beta powers equal bit for bit after each of 10 steps,
    the first ones (a ring smaller than the batch: the no-sample step, the
    tree left alone) included.  The slots themselves equal the restated
    descent over the device's leaves, and every written slot's leaf stays
    1.0."""
    sizes = ORACLE_NETS[net_id]
    E, cap = ORACLE_BATCHES[batch]
    env, net, learner, per, hp = _setup(sizes, inp, dict(batch=batch, tau=0.7, target_update_interval=3, sample_seed=21),
                                        E, cap, dict(alpha=0.0, beta0=0.0, beta_steps=0))
    st, ohp = _state(learner), _ohp(hp)
    W = 2 * env.params.window_radius + 1
    loop = _Loop(env, net, learner, per, inp)
    drawn = {}
    monkeypatch.setattr(O, "sample_indices", lambda seed, step, b, size: drawn[step])
    trained = 0
    for t in range(10):
        if t:
            loop.fill()
        size = per.size
        if size >= batch:
            slots = learner.sample_slots(per)
            torch.cuda.synchronize()
            leaves = _host(per.tree)[per.layout.leaves:]
            assert np.array_equal(_bits(leaves[:size]), _bits(np.ones(size, F))) and not leaves[size:].any()
            drawn[t] = [int(s) for s in _host(slots)]
            assert drawn[t] == R.sample(R.build_tree(leaves), 21, t, batch).tolist(), t
            assert np.array_equal(_bits(_host(per.weights)), _bits(np.ones(batch, F))), t
        else:
            before = _host(per.block) if per.batch else None
        info = O.learner_step(st, ohp, *_ring(per.rb), size, W if inp == "code" else 0)
        trained += info["trained"]
        learner.train(per)
        torch.cuda.synchronize()
        _assert_same(learner, st, t)
        if size < batch:
            assert not info["trained"]
            if before is not None:
                assert np.array_equal(before, _host(per.block)), t  # the tree is left alone
    assert trained >= 7 and learner.counters()["count"] == trained
    assert float(per.pmax.item()) == 1.0
    learner.check_errors()
    after = net.packed.clone()
    net.pack()
    torch.cuda.synchronize()
    assert torch.equal(after, net.packed)  # the act's image is a fresh pack of the online set


def _full_per_run(cap, E, steps, batch=64, boost=()):
    """The full-PER loop; after every step the restatement on the device's
    own slots and weights.  boost: slots whose leaves the test raises to 1e6
    before every step (nearly every row then draws one of them).  Returns
    the number of rows that drew a slot another row drew too."""
    alpha, beta0, beta_steps, eps, seed = 0.6, 0.4, 12, 1e-6, 5
    sizes, inp = (294, 16, 16, 5), "code"
    env, net, learner, per, hp = _setup(sizes, inp, dict(batch=batch, target_update_interval=4, sample_seed=seed),
                                        E, cap, dict(alpha=alpha, beta0=beta0, beta_steps=beta_steps, eps=eps))
    st, ohp = _state(learner), _ohp(hp)
    loop = _Loop(env, net, learner, per, inp)
    P = R.leaves_of(cap)
    leaves = np.zeros(P, F)  # the restated leaves
    pmax = F(1.0)
    dup = trained = 0
    for t in range(steps):
        cursor, size0 = per.cursor, per.size
        loop.fill()
        n_new = min(E, cap)
        leaves[(cursor + np.arange(E)) % cap] = pmax
        size = per.size
        assert size == min(size0 + E, cap) and n_new
        for s in boost:
            per.bind(batch).tree[P + s] = 1e6
            leaves[s] = F(1e6)
        learner.train(per)
        torch.cuda.synchronize()
        tree_dev = _host(per.tree)
        if size >= batch:
            trained += 1
            # the tree the step sampled from: the internal nodes are the rebuild of the leaves before the update
            tree = R.build_tree(leaves)
            assert np.array_equal(_bits(tree_dev[1:P]), _bits(tree[1:P])), t
            slots, w = _host(per.slots), _host(per.weights)
            assert np.array_equal(slots, R.sample(tree, seed, t, batch)), t
            w32 = R.weights64(tree, slots, size, R.beta_of(beta0, beta_steps, t)).astype(F)
            # (loose, w * wmax rounds twice more: the sampler's test pins the weights)
            assert (R.ulps(w * F(per.wmax.item()), w32) <= 4).all(), t
            info = R.per_step(st, ohp, *_ring(per.rb), size, slots, w, 7)
            _assert_same(learner, st, t)
            absd = info["absd"]
            assert np.array_equal(_bits(_host(per.abs_td)), _bits(absd)), t
            # the new leaves: within 1 f32 ulp of the float64 formula on the restatement's |d|; a slot drawn by
            # several rows holds the largest of its rows' values
            p_dev = tree_dev[P + slots]
            p_ref = R.priority32(absd, eps, alpha)
            best = {}
            for s, p in zip(slots.tolist(), p_ref.tolist()):
                best[s] = max(best.get(s, 0.0), p)
            dup += batch - len(best)
            want = np.array([best[s] for s in slots.tolist()], F)
            assert (R.ulps(p_dev, want) <= 1).all(), (t, int((R.ulps(p_dev, want) > 1).sum()))
            leaves[slots] = p_dev  # (the device's own leaves from here: a 1-ulp difference must not compound)
            assert np.array_equal(_bits(tree_dev[P:]), _bits(leaves)), t  # no other leaf moved
            pmax = max(pmax, F(p_dev.max()))
            assert F(per.pmax.item()) == pmax, t
        else:
            R.per_step(st, ohp, *_ring(per.rb), size, None, None, 7)
            _assert_same(learner, st, t)
            assert np.array_equal(_bits(tree_dev[P:]), _bits(leaves)), t
    assert learner.counters()["count"] == trained and trained >= steps - 1
    learner.check_errors()
    return dup


@gpu
def test_full_per_matches_the_restatement():
    """alpha 0.6, beta 0.4 annealed over 12 steps, eps 1e-6; 20 steps at
    batch 64 on a ring of 1000 slots that wraps, 96 rows added per step.
    After every step tests/_per_ref.per_step, given the device's own slots
    and weights of that step, reproduces the four parameter sets and the
    counters bit for bit and the rows' |d|; the slots are the restated
    descent on the rebuilt tree of the device's leaves; the new leaves are
    within 1 f32 ulp of (|d| + eps) ** alpha in float64; no other leaf
    moves; pmax is the running maximum."""
    _full_per_run(cap=1000, E=96, steps=20)


@gpu
def test_a_slot_drawn_twice_takes_the_larger_priority():
    """Four slots share a batch of 64: a ring must hold a batch before the
    learner samples (buffers.py can_sample), so instead of a ring of 4 slots
    the test raises 4 leaves of a 200-slot ring to 1e6 before every step and
    nearly every row draws one of them.  Each drawn leaf then holds the
    largest of its rows' new priorities (the integer max on the floats'
    bits), step after step, with everything else as in
    test_full_per_matches_the_restatement."""
    assert _full_per_run(cap=200, E=50, steps=6, boost=(1, 2, 3, 5)) >= 5 * 50


@gpu
def test_prioritized_learner_is_graph_capturable():
    """PrioritizedDQNLearner.train captured once with torch.cuda.graph and
    replayed 5 times equals 5 eager calls on a twin bit for bit: parameter
    sets, counters, packed image and the whole prioritized block (tree, pmax,
    slots, weights)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams, PrioritizedDQNLearner, PrioritizedReplay, ReplayBuffer
    cap = 900
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), cap)
    env.reset(seed=7)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    acts = env.synth_actions(seed=9, step=0)
    r, d = env.step(acts, code=nxt)
    rb.add_many(cur, acts, r, nxt, d)
    hp = DQNHParams(batch=257, tau=0.6, target_update_interval=3, epsilon_decay_every=2)

    def make():
        net, target = _net_and_target((294, 128, 64, 5), "code", seed=4)
        per = PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=4, batch=257)  # (a ring wrapped when full)
        return net, PrioritizedDQNLearner(net, hp, target=target), per

    (net_e, eager, per_e), (net_g, graphed, per_g) = make(), make()
    torch.cuda.synchronize()
    assert torch.equal(per_e.block, per_g.block) and float(per_e.tree[per_e.layout.leaves:].sum().item()) == cap
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed.train(per_g)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert graphed.counters()["step"] == 0  # (capturing runs nothing)
    for _ in range(5):
        g.replay()
        eager.train(per_e)
    torch.cuda.synchronize()
    assert eager.counters()["step"] == 5 and eager.counters()["count"] == 5
    for k in SETS:
        assert torch.equal(eager.sets[k].view(torch.int32), graphed.sets[k].view(torch.int32)), k
    assert eager.counters() == graphed.counters()
    assert torch.equal(net_e.packed, net_g.packed)
    assert torch.equal(per_e.block, per_g.block)
    assert float(per_e.pmax.item()) >= 1.0 and not torch.equal(per_e.tree[per_e.layout.leaves:],
                                                              torch.ones_like(per_e.tree[per_e.layout.leaves:]))


@gpu
def test_agent_trained_with_prioritized_replay_beats_random(tmp_path):
    """train(EnvParams(), 4096, 300) at batch 256 with prioritized replay
    (alpha 0.6, beta 0.4 annealed over the run), then the greedy eval_jax of
    the learned parameters: drone 0's reward is above the random drones'.
    The saved checkpoint reloads bit-identical to the online set.  Nothing is
    asserted against uniform replay; the figures of both are in
    profiles/per/learning.json (tools/time_per_learn.py --learning)."""
    from dronerl_amd import EnvParams
    from dronerl_amd.checkpoint import load_qnetwork
    from dronerl_amd.dqn import DQNHParams, PrioritizedDQNLearner, PrioritizedReplay, QNetwork
    from dronerl_amd.train import evaluate, train
    p = EnvParams()
    res = train(p, 4096, 300, hp=DQNHParams(batch=256, num_steps=300),
                per=dict(alpha=0.6, beta0=0.4, beta_steps=300, eps=1e-6))
    assert isinstance(res.learner, PrioritizedDQNLearner) and isinstance(res.replay, PrioritizedReplay)
    c = res.learner.counters()
    assert c["step"] == 300 and c["count"] == 300
    assert float(res.replay.pmax.item()) >= 1.0 and float(res.replay.tree[1].item()) > 0
    path = str(tmp_path / "agent.safetensors")
    res.learner.save(path)
    lin = [m for m in load_qnetwork(path).network.children() if isinstance(m, torch.nn.Linear)]
    for (w, b), m in zip(res.learner.params("online"), lin):
        assert torch.equal(w.cpu(), m.weight.detach()) and torch.equal(b.cpu(), m.bias.detach())
    qnet = QNetwork(294, (128, 64), precision="f32")
    qnet.load(*zip(*res.learner.params("online")))
    agent, rnd, table = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
    print(f"eval after 300 steps at batch 256 with prioritized replay: agent {agent[0]:.4f} +- {agent[1]:.4f}, "
          f"random {rnd[0]:.4f} +- {rnd[1]:.4f}, gap {agent[0] - rnd[0]:.4f}")
    assert table.shape == (5, 2)
    assert agent[0] > rnd[0], (agent, rnd)


@gpu
def test_train_main_cli_with_prioritized_replay(tmp_path):
    """`python -m dronerl_amd.train --prioritized_replay` runs end to end,
    saves both checkpoints (which reload to the same parameters) and runs
    the final eval."""
    from dronerl_amd.checkpoint import load_qnetwork, read_checkpoint
    from dronerl_amd.train import main
    m = main(["--num_envs", "512", "--num_steps", "60", "--batch_size", "128", "--prioritized_replay", "--num_evals", "2",
              "--num_eval_steps", "200", "--save_final_checkpoint", "--output_dir", str(tmp_path)])
    assert m["obs_per_sec"] > 0 and m["num_gpus"] == 1
    assert -1.0 <= m["eval_reward_mean"] <= 1.0 and -1.0 <= m["random_reward_mean"] <= 1.0
    nets = []
    for fmt in ("jax", "torch"):
        ck = read_checkpoint(m[f"checkpoint_{fmt}"])
        assert ck.dense_layers == (128, 64) and m[f"checkpoint_{fmt}"].endswith(f"agent_60_steps_{fmt}.safetensors")
        nets.append([x for x in load_qnetwork(m[f"checkpoint_{fmt}"]).network.children()
                     if isinstance(x, torch.nn.Linear)])
    for a, b in zip(*nets):
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
