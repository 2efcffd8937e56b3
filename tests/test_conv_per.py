"""Prioritized replay for the conv and the wide single-agent DQN learners:
drl_convnet_dqn_per_train (dronerl_amd/csrc/convper/),
drl_widenet_dqn_per_train (dronerl_amd/csrc/per/dronerl_per_api.cpp),
dqn.PrioritizedConvDQNLearner, dqn.PrioritizedWideDQNLearner,
dqn.make_per_learner, train(per=...) for conv and wide nets and
`python -m dronerl_amd.per_train`.

What pins the conv learner:
  * tests/_conv_per_ref.py, tests/_conv_learner_ref.py's restatement with
    mean(w * (q_a - td)^2) as the loss, in f64 and f32: the device is
    compared with the f64 one per step, loaded with the device's own state,
    slots and weights; the tolerance comes from the f32 one alone (per tensor
    max(1e-5, 4 x its distance from the f64 one)) and may never exceed 1e-4;
  * tests/_per_ref.py, as it is, for the tree, the draw, the weights and the
    priorities;
  * LargeBatchConvDQNLearner itself: with alpha = 0 and beta = 0 every
    weight is 1.0 and a step equals the uniform learner's on the same rows
    bit for bit.
The wide learner runs the dense prioritized learner's kernels, so it is
pinned as that one is: tests/_per_ref.per_step (the oracle's own arithmetic)
bit for bit.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from oracle import dqn_learner as O
from tests import _conv_learner_ref as R
from tests import _conv_per_ref as RP
from tests import _per_ref as PR
from tests import test_conv_large_batch_learner as CL
from tests import test_prioritized_replay as TP

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TOL_CAP = 1e-4
STEPS = 8
SETS = ("online", "target", "m", "v")
F = np.float32
PER_EPS = 1e-6
vp = ctypes.c_void_p
NETS = CL.NETS

# (net, rows, batch, hyperparameters, ring slots, alpha, beta0): the per-step parity cases; beta anneals to 1 over
# the 8 steps
CASES = [
    ("b", "code", 8, {}, 96, 0.6, 0.4),
    ("a", "obs", 65, dict(epsilon_decay=0.9, epsilon_decay_every=1), 128, 0.6, 0.4),
    ("c", "code", 96, dict(tau=0.6, target_update_interval=3), 300, 1.0, 1.0),
    ("i", "obs", 130, {}, 300, 0.4, 0.0),
    ("h", "code", 257, {}, 300, 0.6, 0.4),
    ("s", "code", 72, dict(learning_rate=5e-4, target_update_interval=100), 300, 0.6, 0.4),  # preloaded moments
]
CASE_IDS = [f"{c[0]}-{c[1]}-{c[2]}" for c in CASES]


def _draw(leaves, seed, step, batch, size, beta0):
    """(tree, slots, weights f32): the numpy draw of a step from the leaves -- _per_ref's tree and descent, its
    float64 weights rounded to f32 and divided by their maximum."""
    tree = PR.build_tree(leaves)
    slots = PR.sample(tree, seed, step, batch)
    w = PR.weights64(tree, slots, size, PR.beta_of(beta0, STEPS, step)).astype(F)
    return tree, slots, (w / w.max()).astype(F)


def _new_leaves(leaves, slots, absd, alpha):
    """The leaves after a step: each drawn slot the largest priority32 of the rows that drew it."""
    out = leaves.copy()
    out[slots] = F(0.0)
    np.maximum.at(out, slots, PR.priority32(absd, PER_EPS, alpha))
    return out


# ------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("bias_std", [0.0, 0.05])
def test_tolerance_condition_holds_on_the_references_alone(case, bias_std):
    """The tolerance the GPU test computes stays within 1e-4: the two
    restatements alone on synthetic windows for exactly the GPU cases, 8
    steps of a numpy PER loop (leaves from 1.0, _per_ref's draw, the weights
    rounded to f32 and divided by their maximum, beta annealed over the 8
    steps, the priorities from the f64 |d| through priority32, the largest
    over duplicates), zero and random biases; the sweep net from its
    preloaded moments."""
    name, _, batch, kw, cap, alpha, beta0 = case
    W, conv, dense = NETS[name]
    hp = CL._ohp(batch, kw)
    seed = sum(map(ord, name)) + CL.SEED_SHIFT.get(name, 0)
    g = np.random.default_rng(seed)
    obs, nxt = R.synthetic_windows(W, cap, seed + 1), R.synthetic_windows(W, cap, seed + 2)
    act = g.integers(0, 5, cap).astype(np.int32)
    rew = g.choice(np.array([0.0, 1.0, -1.0, -0.1], np.float32), cap)
    done = (g.random(cap) < 0.1).astype(np.uint8)
    st = {"online": R.random_params(W, conv, dense, seed + 3, bias_std),
          "target": R.random_params(W, conv, dense, seed + 4, bias_std), "step": 0, "count": 0}
    pre = CL._moments(name, seed + 8)
    st["m"] = pre[0] if pre else [(np.zeros_like(w), np.zeros_like(b)) for w, b in st["online"]]
    st["v"] = pre[1] if pre else [(np.zeros_like(w), np.zeros_like(b)) for w, b in st["online"]]
    leaves = np.zeros(PR.leaves_of(cap), F)
    leaves[:cap] = F(1.0)
    worst = worst_absd = 0.0
    dup = 0
    for step in range(STEPS):
        _, idx, w = _draw(leaves, hp.sample_seed, step, batch, cap, beta0)
        dup = max(dup, batch - len(set(idx.tolist())))
        args = (st, hp, W, conv, obs[idx], nxt[idx], act[idx], rew[idx], done[idx], w)
        r64, r32 = RP.ref_step(*args, torch.float64), RP.ref_step(*args, torch.float32)
        for k in SETS:
            for (a, b), (e, f) in zip(r32[k], r64[k]):
                worst = max(worst, R.tolerance(a, e), R.tolerance(b, f))
        worst = max(worst, R.tolerance(r32["loss"], r64["loss"]), R.tolerance(r32["absd"], r64["absd"]))
        worst_absd = max(worst_absd, float(np.max(np.abs(r32["absd"].astype(np.float64) - r64["absd"]))))
        leaves = _new_leaves(leaves, idx, r64["absd"], alpha)
        for k in SETS:  # the next step starts from f32 state, as the device's does
            st[k] = [(w_.astype(np.float32), b.astype(np.float32)) for w_, b in r64[k]]
        st["step"] += 1
        st["count"] += 1
    print(f"{name}-{batch}: worst tolerance {worst:.3g}, f32 |d| off by {worst_absd:.3g}, up to {dup} duplicate draws")
    assert worst <= TOL_CAP


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind, _bind_convnet, _bind_widenet
    return _bind_widenet(_bind(_bind_convnet(lib())))


def _bad_per_hparams():
    from dronerl_amd.dqn import DrlPerHParams
    return ((DrlPerHParams(-0.1, 0.4, 0, 1e-6), b"alpha"), (DrlPerHParams(float("nan"), 0.4, 0, 1e-6), b"alpha"),
            (DrlPerHParams(0.6, -0.1, 0, 1e-6), b"beta0"), (DrlPerHParams(0.6, 1.5, 0, 1e-6), b"beta0"),
            (DrlPerHParams(0.6, 0.4, -1, 1e-6), b"beta_steps"), (DrlPerHParams(0.6, 0.4, 0, -1e-6), b"eps"))


def _wide_desc(hidden, inp=0):
    from dronerl_amd.dqn import DrlWidenetDesc
    return DrlWidenetDesc(294, len(hidden), (ctypes.c_int32 * 3)(*hidden, *[0] * (3 - len(hidden))), 5, inp)


@pytest.mark.parametrize("family", ["conv", "wide"])
def test_per_train_calls_validate_before_device_work(family):
    """drl_convnet_dqn_per_train and drl_widenet_dqn_per_train refuse, by
    name and before any device work (no GPU needed): NULL and misaligned
    blocks, batch 0 and 4097, a capacity above 2^24, each PER hyperparameter
    out of range, a size outside [0, capacity], a code net with f32 rows, and
    what their uniform learners refuse."""
    from dronerl_amd.dqn import DQNHParams, DrlPerHParams, DrlReplay
    L = _lib()
    err = lambda: L.drl_last_error()  # noqa: E731
    if family == "conv":
        f, d, dc = L.drl_convnet_dqn_per_train, CL._desc("a"), CL._desc("a", "code")
    else:
        f, d, dc = L.drl_widenet_dqn_per_train, _wide_desc((256, 128, 64)), _wide_desc((256, 128, 64), 1)
    hp = DQNHParams(batch=256).c()
    good = DrlPerHParams(0.6, 0.4, 100, 1e-6)
    ring = DrlReplay(5000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def train(desc=d, h=hp, ph=good, agent=vp(1 << 20), packed=vp(1 << 21), r=ring, size=100, per=vp(1 << 23)):
        return f(ctypes.byref(desc), None if h is None else ctypes.byref(h), None if ph is None else ctypes.byref(ph),
                 agent, packed, None if r is None else ctypes.byref(r), size, per, None)
    assert train(h=None) != 0 and b"hparams is NULL" in err()
    assert train(ph=None) != 0 and b"hparams are NULL" in err()
    for h, name in _bad_per_hparams():
        assert train(ph=h) != 0 and name in err(), name
    assert train(agent=None) != 0 and b"agent block" in err()
    assert train(agent=vp((1 << 20) + 8)) != 0 and b"16-byte" in err()
    assert train(packed=None) != 0 and b"packed" in err()
    assert train(packed=vp((1 << 21) + 4)) != 0 and b"16-byte" in err()
    assert train(r=None) != 0 and b"replay" in err()
    assert train(r=DrlReplay(5000, 294, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"NULL" in err()
    assert train(per=None) != 0 and b"prioritized replay block" in err()
    assert train(per=vp((1 << 23) + 4)) != 0 and b"16-byte" in err()
    assert train(size=-1) != 0 and b"size" in err()
    assert train(size=5001) != 0 and b"size" in err()
    big = DrlReplay((1 << 24) + 1, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    assert train(r=big) != 0 and b"capacity must be in [1, 2^24]" in err()
    assert train(desc=dc) != 0 and b"policy code" in err()  # f32 rows for a code net
    assert train(r=DrlReplay(5000, 292, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"obs_floats" in err()
    assert train(r=DrlReplay(5000, 294, (1 << 20) + 2, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0
    assert b"4-byte" in err()
    for batch in (0, 4097):
        assert train(h=DQNHParams(batch=batch).c()) != 0 and b"batch" in err()
    assert train(h=DQNHParams(batch=256, target_update_interval=0).c()) != 0 and b"target_update_interval" in err()
    assert train(h=DQNHParams(batch=256, beta1=1.0).c()) != 0 and b"beta1" in err()
    if family == "conv":
        bad = CL._desc("a")
        bad.conv[0].kernel_size = 6
        assert train(desc=bad) != 0 and b"kernel_size" in err()
    else:
        assert train(desc=_wide_desc((264,))) != 0 and b"hidden" in err()


def test_routing_of_prioritized_learners_and_per_train_cli(monkeypatch):
    """make_per_learner returns the prioritized learner of the net's family
    (the classes stubbed: no device); make_learner(per=True) still refuses
    conv and wide nets; per_train.parse_args takes conv and wide nets, fills
    per_beta_steps from num_steps and refuses --per_beta 1.5 and
    --use_sharding by name; train's own flag keeps its refusals."""
    from dronerl_amd import dqn, per_train, train
    made = []
    for name in ("PrioritizedDQNLearner", "PrioritizedWideDQNLearner", "PrioritizedConvDQNLearner"):
        monkeypatch.setattr(dqn, name, lambda net, hp, _n=name, **kw: made.append((_n, hp.batch, kw)) or _n)
    nets = ((dqn.QNetwork, "PrioritizedDQNLearner"), (dqn.WideQNetwork, "PrioritizedWideDQNLearner"),
            (dqn.ConvQNetwork, "PrioritizedConvDQNLearner"))
    for cls, want in nets:
        for batch in (1, 64, 65, 4096):
            assert dqn.make_per_learner(cls.__new__(cls), dqn.DQNHParams(batch=batch), generator=None) == want
            assert made[-1] == (want, batch, {"generator": None})
    assert dqn.make_per_learner(dqn.ConvQNetwork.__new__(dqn.ConvQNetwork)) == "PrioritizedConvDQNLearner"
    monkeypatch.undo()
    for cls in (dqn.WideQNetwork, dqn.ConvQNetwork):
        with pytest.raises(ValueError, match="prioritized replay trains dense nets of hidden widths up to 128"):
            dqn.make_learner(cls.__new__(cls), dqn.DQNHParams(), per=True)
    assert issubclass(dqn.PrioritizedConvDQNLearner, dqn.LargeBatchConvDQNLearner)
    assert issubclass(dqn.PrioritizedWideDQNLearner, dqn.WideDQNLearner)
    for cls in (dqn.PrioritizedConvDQNLearner, dqn.PrioritizedWideDQNLearner):
        with pytest.raises(ValueError, match="takes a PrioritizedReplay"):
            cls.train(object.__new__(cls), object())
        with pytest.raises(ValueError, match="takes a PrioritizedReplay"):
            cls.sample_slots(object.__new__(cls), object())
    a = per_train.parse_args(["--network_type", "conv", "--num_steps", "500", "--batch_size", "72"])
    assert a.network_type == "conv" and a.prioritized_replay and a.batch_size == 72
    assert train.per_options_of(a) == dict(alpha=0.6, beta0=0.4, beta_steps=500, eps=1e-6)
    a = per_train.parse_args(["--hidden_layers", "256", "128", "64", "--per_alpha", "0.5", "--per_beta", "0.7",
                              "--per_beta_steps", "0", "--per_eps", "1e-3", "--prioritized_replay"])
    assert tuple(a.hidden_layers) == (256, 128, 64)
    assert train.per_options_of(a) == dict(alpha=0.5, beta0=0.7, beta_steps=0, eps=1e-3)
    assert train.per_options_of(per_train.parse_args([])) == dict(alpha=0.6, beta0=0.4, beta_steps=1000, eps=1e-6)
    with pytest.raises(ValueError, match="per_beta"):
        per_train.parse_args(["--per_beta", "1.5"])
    with pytest.raises(ValueError, match="per_alpha"):
        per_train.parse_args(["--network_type", "conv", "--per_alpha", "-1"])
    with pytest.raises(ValueError, match="per_train with --use_sharding"):
        per_train.parse_args(["--use_sharding", "--num_envs", "8"])
    with pytest.raises(ValueError, match="--prioritized_replay with --network_type conv"):
        train.parse_args(["--prioritized_replay", "--network_type", "conv"])


# Every __global__ kernel under csrc/convper/ and the -m gpu test that launches it.
_T = "test_conv_per.py::"
KERNEL_TESTS = {
    "drl_convnet_dqn_per_rows_kernel": _T + "test_learner_matches_the_restatement_per_step",
    "drl_convnet_dqn_per_priority_kernel": _T + "test_a_slot_drawn_twice_takes_the_larger_priority",
}


def test_every_convper_kernel_has_a_gpu_test():
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "convper", "*.hip")):
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
_host = CL._host


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _ohp_of(hp):
    return O.HParams(batch=hp.batch, gamma=hp.gamma, learning_rate=hp.learning_rate, beta1=hp.beta1, beta2=hp.beta2,
                     adam_eps=hp.adam_eps, tau=hp.tau, target_update_interval=hp.target_update_interval,
                     epsilon_decay=hp.decay(), epsilon_end=hp.epsilon_end,
                     epsilon_decay_every=hp.epsilon_decay_every, sample_seed=hp.sample_seed)


def _conv_learner(name, inp, batch, kw, **more):
    from dronerl_amd.dqn import PrioritizedConvDQNLearner
    net, learner, hp = CL._learner(name, inp, batch, kw, cls=PrioritizedConvDQNLearner, **more)
    assert type(learner) is PrioritizedConvDQNLearner
    return net, learner, hp


@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_learner_matches_the_restatement_per_step(case):
    """8 prioritized learner steps on a filled, wholly marked ring of real
    windows.  At every step: the slots equal _per_ref.sample on the tree
    rebuilt from the device's leaves; the weights are within 1 ulp of the
    float64 weights rounded to f32 over their maximum; the f64 and f32
    restatements, loaded with the device's pre-step state and the device's
    slots and weights, bound the four sets, the loss and |d| by the derived
    tolerance (never above 1e-4); the drawn slots' new leaves are
    priority32(device |d|), the largest over the rows that drew the slot,
    bit for bit, no other leaf moves and pmax is the running maximum; the
    schedule is exact."""
    from dronerl_amd.dqn import PrioritizedReplay
    name, inp, batch, kw, cap, alpha, beta0 = case
    W, conv, dense = NETS[name]
    rb, host = CL._ring(W, inp, cap)
    net, learner, hp = _conv_learner(name, inp, batch, kw, bias_std=0.0 if name == "b" else 0.05)
    per = PrioritizedReplay(rb, alpha=alpha, beta0=beta0, beta_steps=STEPS, eps=PER_EPS, batch=batch)
    ohp = _ohp_of(hp)
    P = per.layout.leaves
    torch.cuda.synchronize()
    leaves = _host(per.tree)[P:]
    assert np.array_equal(leaves[:cap], np.ones(cap, F)) and not leaves[cap:].any()
    pmax = F(1.0)
    worst_tol = worst = 0.0
    dup = 0
    for step in range(STEPS):
        st = CL._state(learner)
        assert st["step"] == step and st["count"] == step
        learner.train(per)
        dev = CL._state(learner)
        tree_dev, slots, w_dev = _host(per.tree), _host(per.slots), _host(per.weights)
        absd_dev = _host(per.abs_td)
        tree, want, w_ref = _draw(leaves, hp.sample_seed, step, batch, rb.size, beta0)
        assert np.array_equal(_bits(tree_dev[1:P]), _bits(tree[1:P])), step  # the tree the step drew from
        assert np.array_equal(slots, want), step
        assert (PR.ulps(w_dev, w_ref) <= 1).all(), (step, int(PR.ulps(w_dev, w_ref).max()))
        assert w_dev.max() == F(1.0) and (w_dev > 0).all()
        dup = max(dup, batch - len(set(slots.tolist())))
        X, Xn = CL._rows(host, slots, W, inp)
        args = (st, ohp, W, conv, X, Xn, host["actions"][slots], host["rewards"][slots], host["dones"][slots], w_dev)
        r64, r32 = RP.ref_step(*args, torch.float64), RP.ref_step(*args, torch.float32)
        for what, got in (("loss", dev["loss"]), ("absd", absd_dev)):
            tol, dist = R.tolerance(r32[what], r64[what]), R.rel(got, r64[what])
            print(f"{name}-{batch} step {step}: {what} distance {dist:.3g}, tolerance {tol:.3g}")
            assert tol <= TOL_CAP and dist <= tol, (step, what, dist, tol)
        for k in SETS:
            for l, ((a, b), (e32, f32), (e, f)) in enumerate(zip(dev[k], r32[k], r64[k])):
                for what, got, lo, hi in (("W", a, e32, e), ("b", b, f32, f)):
                    tol, dist = R.tolerance(lo, hi), R.rel(got, hi)
                    worst_tol, worst = max(worst_tol, tol), max(worst, dist)
                    assert tol <= TOL_CAP and dist <= tol, (step, k, l, what, dist, tol)
        # the priorities: the device's own |d| through the float64 formula, the largest over duplicates
        new = _new_leaves(leaves, slots, absd_dev, alpha)
        assert np.array_equal(_bits(tree_dev[P:]), _bits(new)), step
        pmax = max(pmax, F(PR.priority32(absd_dev, PER_EPS, alpha).max()))
        assert F(per.pmax.item()) == pmax, step
        leaves = new
        # the schedule, exactly
        assert dev["step"] == step + 1 and dev["count"] == step + 1
        eps = np.float32(st["epsilon"])
        if step % hp.epsilon_decay_every == 0:
            eps = max(np.float32(eps * np.float32(hp.decay())), np.float32(hp.epsilon_end))
        assert np.float32(dev["epsilon"]) == eps, step
        assert dev["beta1_pow"] == st["beta1_pow"] * hp.beta1 and dev["beta2_pow"] == st["beta2_pow"] * hp.beta2
    print(f"{name}-{batch}: worst distance {worst:.3g}, worst tolerance {worst_tol:.3g}, up to {dup} duplicate draws")
    learner.check_errors()
    net.check_errors()


@gpu
@pytest.mark.parametrize("name,batch", [("b", 65), ("c", 257)])
def test_alpha0_beta0_is_the_uniform_conv_learner_bit_exact(name, batch):
    """alpha = 0 and beta = 0, device against device, 6 steps on code rows:
    per step the drawn slots are read, a LargeBatchConvDQNLearner is given a
    sample seed whose uniform draw over a 65,536-slot comparison ring has no
    repeated index, that ring is filled so that its drawn slots hold the
    prioritized ring's drawn rows, and the prioritized learner's whole agent
    block is copied into it (both use one layout query); after one step of
    each the four sets, the counters (the loss among them) and the packed
    image are byte-identical, every weight and every new leaf exactly 1.0."""
    from dronerl_amd.dqn import LargeBatchConvDQNLearner, PrioritizedReplay, ReplayBuffer
    W = NETS[name][0]
    kw = dict(tau=0.6, target_update_interval=3)
    rb, _ = CL._ring(W, "code", 300)
    net, learner, hp = _conv_learner(name, "code", batch, kw)
    per = PrioritizedReplay(rb, alpha=0.0, beta0=0.0, beta_steps=0, batch=batch)
    big = 65536
    twin_rb = ReplayBuffer(big, W * W * 6, torch.device("cuda"), code_radius=(W - 1) // 2)
    twin_rb.size = big
    P = per.layout.leaves
    ones = np.zeros(P, F)
    ones[:300] = F(1.0)
    for step in range(6):
        slots = learner.sample_slots(per)
        assert np.array_equal(_host(slots), PR.sample(PR.build_tree(ones), hp.sample_seed, step, batch)), step
        seed = 1000
        while len(set(O.sample_indices(seed, step, batch, big))) < batch:
            seed += 1
        assert seed < 1050
        idx = torch.tensor(O.sample_indices(seed, step, batch, big), device="cuda")
        for k in ("obs", "next_obs", "actions", "rewards", "dones"):
            getattr(twin_rb, k)[idx] = getattr(rb, k)[slots]
        tnet, twin, _ = CL._learner(name, "code", batch, dict(kw, sample_seed=seed), cls=LargeBatchConvDQNLearner)
        assert type(twin) is LargeBatchConvDQNLearner and twin.block.numel() == learner.block.numel()
        twin.block.copy_(learner.block)
        tnet.packed.copy_(net.packed)
        assert twin.sample_slots(big).tolist() == idx.tolist()
        twin.train(twin_rb)
        learner.train(per)
        torch.cuda.synchronize()
        assert CL._same(learner, twin), step
        assert torch.equal(learner._ctr_f.view(torch.int32), twin._ctr_f.view(torch.int32)), step
        c = learner.counters()
        assert c["step"] == step + 1 and c["count"] == step + 1 and c["loss"] > 0.0
        assert np.array_equal(_bits(_host(per.weights)), _bits(np.ones(batch, F))), step
        assert np.array_equal(_bits(_host(per.tree)[P:]), _bits(ones)), step
        assert float(per.pmax.item()) == 1.0
    learner.check_errors()


@gpu
def test_a_slot_drawn_twice_takes_the_larger_priority():
    """Four slots share a batch of 8 (net b).  A ring must hold a batch
    before the learner samples (buffers.py can_sample: with size < batch
    nothing is drawn), so a ring of 4 slots can never train at batch 8;
    instead the ring has 8 written slots of which only 4 carry a priority
    (the test zeroes the other four leaves, and the descent never enters a
    node of value 0.0).  From equal leaves every one of the 4 slots is drawn
    exactly twice; over 4 steps every slot with a priority is drawn at least
    twice, each drawn leaf ends at the largest of its rows' priorities (the
    integer max on the floats' bits), no other leaf moves and pmax
    follows."""
    from dronerl_amd.dqn import PrioritizedReplay, ReplayBuffer
    alpha = 0.6
    src, _ = CL._ring(7, "code", 300)
    rb = ReplayBuffer(8, 294, torch.device("cuda"), code_radius=3)
    for k in ("obs", "next_obs", "actions", "rewards", "dones"):
        getattr(rb, k).copy_(getattr(src, k)[10:18])
    rb.size = 8
    net, learner, hp = _conv_learner("b", "code", 8, {}, bias_std=0.0)
    per = PrioritizedReplay(rb, alpha=alpha, beta0=0.4, beta_steps=4, eps=PER_EPS, batch=8)
    P = per.layout.leaves
    assert P == 8
    per.tree[P + 4:].zero_()
    torch.cuda.synchronize()
    leaves = _host(per.tree)[P:]
    assert np.array_equal(leaves, np.array([1, 1, 1, 1, 0, 0, 0, 0], F))
    pmax = F(1.0)
    for step in range(4):
        learner.train(per)
        torch.cuda.synchronize()
        slots, absd = _host(per.slots), _host(per.abs_td)
        assert np.array_equal(slots, PR.sample(PR.build_tree(leaves), hp.sample_seed, step, 8)), step
        counts = np.bincount(slots, minlength=8)
        assert not counts[4:].any() and counts.max() >= 2, (step, counts)
        if step == 0:
            assert (counts[:4] == 2).all(), counts
        p = PR.priority32(absd, PER_EPS, alpha)
        new = _new_leaves(leaves, slots, absd, alpha)
        for s in range(4):
            if counts[s]:
                assert new[s] == p[slots == s].max()
        assert np.array_equal(_bits(_host(per.tree)[P:]), _bits(new)), step
        pmax = max(pmax, F(p.max()))
        assert F(per.pmax.item()) == pmax, step
        leaves = new
    assert learner.counters()["count"] == 4
    learner.check_errors()


@gpu
def test_without_a_sample_the_tree_is_left_alone():
    """size < batch: the prioritized block (tree, slots, weights, pmax) is
    byte-unchanged and the step is LargeBatchConvDQNLearner's no-sample step
    bit for bit -- the target blend when due, step and epsilon advance, count
    and loss stay 0."""
    from dronerl_amd.dqn import LargeBatchConvDQNLearner, PrioritizedReplay
    rb, _ = CL._ring(7, "obs", 300)  # 300 slots < 512 rows
    kw = dict(tau=0.25, epsilon_decay_every=1)
    net, learner, hp = _conv_learner("a", "obs", 512, kw)
    _, twin, _ = CL._learner("a", "obs", 512, kw, cls=LargeBatchConvDQNLearner)
    per = PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=4, batch=512)
    torch.cuda.synchronize()
    before, target0 = per.block.clone(), learner.sets["target"].clone()
    assert float(per.tree[per.layout.leaves:].sum().item()) == 300.0 and CL._same(learner, twin)
    for step in range(2):
        learner.train(per)
        twin.train(rb)
        torch.cuda.synchronize()
        assert CL._same(learner, twin), step
        assert torch.equal(learner._ctr_f.view(torch.int32), twin._ctr_f.view(torch.int32)), step
        assert torch.equal(before, per.block), step
    c = learner.counters()
    assert c["step"] == 2 and c["count"] == 0 and c["loss"] == 0.0
    assert np.float32(c["epsilon"]) == np.float32(np.float32(np.float32(hp.decay()) * np.float32(hp.decay())))
    assert not torch.equal(target0, learner.sets["target"])  # (the blend of step 0)
    learner.check_errors()


@gpu
def test_prioritized_conv_learner_is_reproducible_and_graph_capturable():
    """Net a at batch 130 behind a fused env step that adds to the ring and
    marks the new rows: act, step + add + mark, train captured once with
    torch.cuda.graph and replayed 5 times equals 5 eager steps of a twin byte
    for byte -- the agent block, the prioritized block (tree, pmax, slots,
    weights), the ring and the packed image.  (The ring's cursor is a host
    value: every step writes the same slots, in the eager twin too.)"""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import PrioritizedReplay, ReplayBuffer
    E, cap = 160, 600

    def fresh():
        env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=3), E)
        env.reset(seed=7)
        env.refill_every = 0  # (the refill cadence is a host counter: off, for both twins)
        rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
        net, learner, _ = _conv_learner("a", "code", 130, dict(tau=0.6, target_update_interval=3,
                                                              epsilon_decay_every=2))
        per = PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=4, batch=130)
        cur, nxt = env.new_code(), env.new_code()
        env.get_code(out=cur)
        acts = torch.zeros((E, 8), dtype=torch.int32, device="cuda")
        rew = torch.empty((E, 8), dtype=torch.float32, device="cuda")
        don = torch.empty((E, 8), dtype=torch.uint8, device="cuda")

        def step():
            net.act(cur, learner.epsilon, seed=3, step=9, actions=acts)
            rb.cursor, rb.size = c0, s0
            env.step(acts, rewards=rew, dones=don, code=nxt, replay=per, replay_obs=cur, synth=(5, 9))
            learner.train(per)
            cur.copy_(nxt)

        c0, s0 = 0, 0
        step()  # (160 rows: the ring holds a batch from here on)
        c0, s0 = rb.cursor, rb.size
        return env, net, learner, per, step

    env_e, net_e, eager, per_e, step_e = fresh()
    env_g, net_g, graphed, per_g, step_g = fresh()
    torch.cuda.synchronize()
    assert eager.counters()["count"] == 1 and torch.equal(per_e.block, per_g.block)
    assert torch.equal(eager.block, graphed.block)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step_g()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert graphed.counters()["step"] == 1  # (capturing runs nothing)
    for _ in range(5):
        g.replay()
        step_e()
    torch.cuda.synchronize()
    assert eager.counters()["step"] == 6 and eager.counters()["count"] == 6
    assert eager.counters() == graphed.counters()
    assert torch.equal(eager.block, graphed.block)
    assert torch.equal(per_e.block, per_g.block)
    assert torch.equal(net_e.packed, net_g.packed)
    for k in ("obs", "next_obs", "actions", "rewards", "dones"):
        assert torch.equal(getattr(per_e.rb, k), getattr(per_g.rb, k)), k
    leaves = per_e.tree[per_e.layout.leaves:]
    assert float(per_e.pmax.item()) >= 1.0 and float(leaves[320:].sum().item()) == 0.0
    assert not torch.equal(leaves[:320], torch.ones_like(leaves[:320]))
    env_e.check_errors()
    env_g.check_errors()
    eager.check_errors()


# ---- the wide agent ----------------------------------------------------------------------------------------
WIDE_NETS = {"256-128-64": (256, 128, 64), "136": (136,)}


def _wide(hidden, inp, batch, per_kw, seed=0, cls=None, net_cls=None):
    """(net, learner, per, hp, rb): a dense net on the 7 x 7 window with random biases and its own target, a
    prioritized learner and a prioritized view of the shared ring of 300 real rows."""
    from dronerl_amd.dqn import DQNHParams, PrioritizedReplay, PrioritizedWideDQNLearner, WideQNetwork
    rb, _ = CL._ring(7, inp, 300)
    g = torch.Generator().manual_seed(seed + 5)
    net = (net_cls or WideQNetwork)(294, hidden, generator=g, input=inp)
    gb = torch.Generator(device="cuda").manual_seed(seed + 6)
    for b in net.biases:
        b.normal_(0, 0.05, generator=gb)
    net.pack()
    target = ([torch.randn(w.shape, generator=g) * 0.1 for w in net.weights],
              [torch.randn(b.shape, generator=g) * 0.05 for b in net.biases])
    hp = DQNHParams(batch=batch, tau=0.7, target_update_interval=3, sample_seed=21)
    learner = (cls or PrioritizedWideDQNLearner)(net, hp, target=target)
    return net, learner, PrioritizedReplay(rb, batch=batch, **per_kw), hp, rb


@gpu
@pytest.mark.parametrize("inp", ["code", "obs"])
@pytest.mark.parametrize("batch", [8, 257])
@pytest.mark.parametrize("net_id", list(WIDE_NETS))
def test_wide_learner_is_the_restatement_bit_exact(net_id, batch, inp):
    """drl_widenet_dqn_per_train on 294-256-128-64-5 and 294-136-5, code and
    f32 rows, batches 8 and 257, against tests/_per_ref.per_step (the
    oracle's own arithmetic) bit for bit: 3 steps with alpha = 0 and beta =
    0, where every weight and every leaf stays exactly 1.0, then 6 steps of a
    fresh learner with alpha 0.6 and beta 0.4 on the device's own slots and
    weights -- the four sets, the counters, |d|; the slots are the restated
    descent, the new leaves priority32(|d|) (the largest over duplicates) bit
    for bit, no other leaf moves, pmax is the running maximum."""
    from dronerl_amd.dqn import PrioritizedWideDQNLearner
    hidden = WIDE_NETS[net_id]
    W = 7 if inp == "code" else 0
    for alpha, beta0, beta_steps, steps in ((0.0, 0.0, 0, 3), (0.6, 0.4, 6, 6)):
        net, learner, per, hp, rb = _wide(hidden, inp, batch, dict(alpha=alpha, beta0=beta0, beta_steps=beta_steps,
                                                                   eps=PER_EPS))
        assert type(learner) is PrioritizedWideDQNLearner
        st, ohp, ring = TP._state(learner), TP._ohp(hp), TP._ring(rb)
        P = per.layout.leaves
        torch.cuda.synchronize()
        leaves = _host(per.tree)[P:]
        pmax = F(1.0)
        for t in range(steps):
            learner.train(per)
            torch.cuda.synchronize()
            tree_dev, slots, w = _host(per.tree), _host(per.slots), _host(per.weights)
            tree = PR.build_tree(leaves)
            assert np.array_equal(slots, PR.sample(tree, 21, t, batch)), t
            if alpha == 0.0:
                assert np.array_equal(_bits(w), _bits(np.ones(batch, F))), t
            else:
                w32 = PR.weights64(tree, slots, rb.size, PR.beta_of(beta0, beta_steps, t)).astype(F)
                assert (PR.ulps(w, (w32 / w32.max()).astype(F)) <= 1).all(), t
            info = PR.per_step(st, ohp, *ring, rb.size, slots, w, W)
            TP._assert_same(learner, st, (alpha, t))
            assert np.array_equal(_bits(_host(per.abs_td)), _bits(info["absd"])), t
            new = _new_leaves(leaves, slots, info["absd"], alpha)
            assert np.array_equal(_bits(tree_dev[P:]), _bits(new)), t
            pmax = max(pmax, F(PR.priority32(info["absd"], PER_EPS, alpha).max()))
            assert F(per.pmax.item()) == pmax, t
            leaves = new
        if alpha == 0.0:
            assert np.array_equal(_bits(leaves[:300]), _bits(np.ones(300, F))) and pmax == F(1.0)
        learner.check_errors()
        after = net.packed.clone()
        net.pack()
        torch.cuda.synchronize()
        assert torch.equal(after, net.packed)  # the act's image is a fresh wide pack of the online set


@gpu
@pytest.mark.parametrize("batch", [8, 257])
def test_wide_entry_point_on_a_narrow_net_is_the_dense_prioritized_learner(batch):
    """A 128-64 net through drl_widenet_dqn_per_train: after each of 5 steps
    the whole agent block and the prioritized block are byte-identical to
    drl_dqn_per_train's on a QNetwork with the same parameters."""
    from dronerl_amd.dqn import PrioritizedDQNLearner, QNetwork
    per_kw = dict(alpha=0.6, beta0=0.4, beta_steps=5, eps=PER_EPS)
    _, wide, per_w, _, _ = _wide((128, 64), "code", batch, per_kw)
    _, dense, per_d, _, _ = _wide((128, 64), "code", batch, per_kw, cls=PrioritizedDQNLearner,
                                  net_cls=lambda *a, **k: QNetwork(*a, precision="f32", **k))
    assert wide.block.numel() == dense.block.numel()
    for t in range(5):
        wide.train(per_w)
        dense.train(per_d)
        torch.cuda.synchronize()
        assert torch.equal(wide.block, dense.block), t
        assert torch.equal(per_w.block, per_d.block), t
    assert wide.counters()["count"] == 5


# ---- end to end ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("net_args", [["--network_type", "conv"], ["--hidden_layers", "256", "128", "64"]],
                         ids=["conv", "wide"])
def test_per_train_main_cli(net_args, tmp_path):
    """`python -m dronerl_amd.per_train` with a conv net and with a wide net
    runs end to end through the family's prioritized learner, saves both
    checkpoints, which reload to the same parameters, and runs the final
    eval."""
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.per_train import main
    m = main([*net_args, "--num_envs", "64", "--num_steps", "60", "--batch_size", "72", "--num_evals", "2",
              "--num_eval_steps", "200", "--save_final_checkpoint", "--output_dir", str(tmp_path)])
    assert m["obs_per_sec"] > 0 and m["num_gpus"] == 1
    assert -1.0 <= m["eval_reward_mean"] <= 1.0 and -1.0 <= m["random_reward_mean"] <= 1.0
    nets = []
    for fmt in ("jax", "torch"):
        ck = read_checkpoint(m[f"checkpoint_{fmt}"])
        assert m[f"checkpoint_{fmt}"].endswith(f"agent_60_steps_{fmt}.safetensors")
        assert ck.network_type == ("conv" if net_args[0] == "--network_type" else "dense")
        nets.append(to_qnet(ck, device="cuda"))
    a, b = nets
    for x, y in zip((*getattr(a, "conv_weights", ()), *a.weights, *getattr(a, "conv_biases", ()), *a.biases),
                    (*getattr(b, "conv_weights", ()), *b.weights, *getattr(b, "conv_biases", ()), *b.biases)):
        assert torch.equal(x, y)


@gpu
def test_conv_agent_trained_with_prioritized_replay_beats_the_random_drone(tmp_path):
    """train(per=..., network_type="conv") at batch 256, 300 steps of 4,096
    envs (alpha 0.6, beta 0.4 annealed over the run): every step trained, the
    saved checkpoint reloads bit-identical to the online set, and the greedy
    agent's mean reward is above the random drone's by what
    test_conv_agent_trained_at_batch_256_beats_the_random_drone asserts of the
    uniform learner.  Nothing is asserted against uniform replay; both runs'
    figures are in profiles/conv_per/learning.json."""
    from dronerl_amd import EnvParams
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import ConvQNetwork, DQNHParams, PrioritizedConvDQNLearner, PrioritizedReplay
    from dronerl_amd.train import evaluate, train
    p = EnvParams(n_drones=4, grid_size=9)
    res = train(p, 4096, 300, network_type="conv", hp=DQNHParams(batch=256, num_steps=300),
                per=dict(alpha=0.6, beta0=0.4, beta_steps=300))
    assert type(res.learner) is PrioritizedConvDQNLearner and isinstance(res.replay, PrioritizedReplay)
    c = res.learner.counters()
    assert c["step"] == 300 and c["count"] == 300 and 0.01 <= c["epsilon"] < 1.0 and np.isfinite(c["loss"])
    assert float(res.replay.pmax.item()) >= 1.0 and float(res.replay.tree[1].item()) > 0
    res.learner.check_errors()
    path = str(tmp_path / "agent.safetensors")
    res.learner.save(path)
    back = to_qnet(read_checkpoint(path), device="cuda")
    for x, y in zip((*back.conv_weights, *back.conv_biases, *back.weights, *back.biases),
                    (*res.net.conv_weights, *res.net.conv_biases, *res.net.weights, *res.net.biases)):
        assert torch.equal(x, y)
    qnet = ConvQNetwork(res.net.obs_shape, res.net.conv_layers, res.net.dense_layers)
    qnet.load(res.net.conv_weights, res.net.conv_biases, res.net.weights, res.net.biases)
    agent, rnd, table = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
    print(f"eval after 300 steps at batch 256 with prioritized replay: agent {agent[0]:.4f} +- {agent[1]:.4f}, "
          f"random {rnd[0]:.4f} +- {rnd[1]:.4f}, gap {agent[0] - rnd[0]:.4f}")
    assert table.shape == (5, 2)
    assert agent[0] > rnd[0] + 0.0692, (agent, rnd)
