"""Double DQN targets (van Hasselt et al. 2016) for the dense learners' launch
chains: drl_dqn_double_train, drl_widenet_dqn_double_train and their
prioritized variants (dronerl_amd/csrc/doubledqn/), DQNHParams.double_dqn,
dqn.make_learner and `python -m dronerl_amd.train --double_dqn`.

Reference: tests/_double_ref.double_step, oracle.learner_step's block (or
tests/_per_ref.per_step's) built from the oracle's own pieces with the
selection rule  a* = first argmax Q_online(next_obs), td = r + gamma qt[a*].
It is pinned here on the CPU twice: with double=False it IS the oracle (bit
for bit), and with double=True it agrees with an independent fp32 PyTorch
restatement (autograd + Adam from the formula) within the tolerance the oracle
itself is pinned with.  The GPU calls must equal it BIT FOR BIT.

The data discriminates: on every net and ring below at least a quarter of a
step's rows select another action than the target's own maximum AND take
another value for it (test_reference_data_discriminates_the_two_rules), so a
kernel that ran the max rule could not pass.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import dqn_learner as O
from tests import _double_ref as D
from tests import _per_ref as R

gpu = pytest.mark.gpu
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SETS = ("online", "target", "m", "v")
REL_TOL = 2e-5  # the tolerance oracle/dqn_learner.py is pinned with (tests/test_dqn_learner.py)
CAP = 300       # every ring here: 300 rows, full

# hidden widths around the 16-unit tile of the forward kernel: below one tile, one tile, a tile and a half with
# three hidden layers, the default net
NETS = {"h8": (8,), "h16-16": (16, 16), "h24-16-8": (24, 16, 8), "h128-64": (128, 64)}
BATCHES = (1, 8, 64, 65)  # (64 rows = one row tile, 65 = two)
STEP_KW = dict(tau=0.5, target_update_interval=3, sample_seed=13, epsilon_decay=0.97, epsilon_decay_every=2)


# ------------------------------------------------------------- host data ---
@functools.lru_cache(maxsize=None)
def host_ring(kind):
    """A full ring of CAP transitions on the host (shared, read only).
    "f32": rows of 150 binary inputs; "code": policy-code rows of a 7x7
    window (128 bytes: a u16 per cell, object code | air << 3, in four groups
    of 13 cells padded to 16; oracle.decode_code_rows reads them)."""
    g = np.random.default_rng(5 if kind == "f32" else 6)
    if kind == "f32":
        obs = (g.random((CAP, 150)) < 0.3).astype(F)
        nxt = (g.random((CAP, 150)) < 0.3).astype(F)
    else:
        def codes():
            obj = g.choice(np.array([0, 0, 0, 2, 3, 4, 5], np.uint16), (CAP, 4, 16))
            air = np.where(g.random((CAP, 4, 16)) < 0.15,
                           (1 + g.integers(0, 101, (CAP, 4, 16))) | (g.integers(0, 2, (CAP, 4, 16)) << 7), 0)
            h = (obj | (air.astype(np.uint16) << 3)).astype(np.uint16)
            h[:, :, 13:] = 0   # (the groups' pad cells)
            h[:, 3, 10:] = 0   # (49 cells: the last group holds 10)
            return np.ascontiguousarray(h).view(np.uint8).reshape(CAP, 128)
        obs, nxt = codes(), codes()
    return {"kind": kind, "n_in": 150 if kind == "f32" else 294, "window": 0 if kind == "f32" else 7,
            "obs": obs, "next_obs": nxt, "actions": g.integers(0, 5, CAP).astype(np.int32),
            "rewards": g.normal(0, 1, CAP).astype(F), "dones": (g.random(CAP) < 0.2).astype(np.uint8)}


def _ring_args(ring):
    return ring["obs"], ring["next_obs"], ring["actions"], ring["rewards"], ring["dones"]


def host_nets(n_in, hidden, n_actions, seed=0):
    """(online, target): [(W [out][in], b [out])] f32, independently
    initialised with the reference's initialisers (dqn.flax_kernel_init:
    he_normal hidden layers, lecun_normal head) and small random biases."""
    from dronerl_amd.dqn import flax_kernel_init
    sizes = [n_in, *hidden, n_actions]
    out = []
    for s in (seed + 100, seed + 200):
        g = torch.Generator().manual_seed(s)
        out.append([(flax_kernel_init((sizes[i + 1], sizes[i]), 2.0 if i < len(sizes) - 2 else 1.0, g).numpy().copy(),
                     (torch.randn(sizes[i + 1], generator=g) * 0.05).numpy().copy())
                    for i in range(len(sizes) - 1)])
    return out[0], out[1]


def ohp(batch, **kw):
    return O.HParams(batch=batch, **{**STEP_KW, **kw})


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same_state(a, b):
    for k in SETS:
        for (w, x), (v, y) in zip(getattr(a, k), getattr(b, k)):
            if not (np.array_equal(_bits(w), _bits(v)) and np.array_equal(_bits(x), _bits(y))):
                return False
    return (a.step, a.count, a.beta1_pow, a.beta2_pow) == (b.step, b.count, b.beta1_pow, b.beta2_pow) and \
        _bits(a.epsilon) == _bits(b.epsilon) and _bits(a.loss) == _bits(b.loss)


# ------------------------------------------------------------------- CPU ---
def test_reference_with_double_off_is_the_oracle_bit_for_bit():
    """double_step(double=False) == oracle.learner_step on the uniform draw,
    and == _per_ref.per_step on given slots and weights: five steps on net
    16-16 at batch 8, all four sets, the loss and the counters on bits."""
    ring, hp = host_ring("f32"), ohp(8)
    online, target = host_nets(150, (16, 16), 5)
    a, b = O.LearnerState.start(online, target, 1.0), O.LearnerState.start(online, target, 1.0)
    for t in range(5):
        ia = D.double_step(a, hp, *_ring_args(ring), CAP, double=False)
        ib = O.learner_step(b, hp, *_ring_args(ring), CAP, 0)
        assert ia["rows"] == ib["rows"] and _bits(ia["loss"]) == _bits(ib["loss"]) and _same_state(a, b), t
    ring = host_ring("code")
    online, target = host_nets(294, (16, 16), 5)
    a, b = O.LearnerState.start(online, target, 1.0), O.LearnerState.start(online, target, 1.0)
    g = np.random.default_rng(3)
    for t in range(5):
        slots, w = g.integers(0, CAP, 8), g.random(8).astype(F)
        ia = D.double_step(a, hp, *_ring_args(ring), CAP, slots=slots, weights=w, code_window=7, double=False)
        ib = R.per_step(b, hp, *_ring_args(ring), CAP, slots, w, 7)
        assert np.array_equal(_bits(ia["absd"]), _bits(ib["absd"])) and _same_state(a, b), t


def _torch_forward(ps, X):
    a = X
    for i in range(0, len(ps), 2):
        a = a @ ps[i].t() + ps[i + 1]
        if i < len(ps) - 2:
            a = torch.relu(a)
    return a


def _torch_double_step(ts, hp, X, Xn, act, rew, done):
    """fp32 PyTorch restatement of the Double DQN train_step + optax.adam,
    independent of the oracle's order: autograd for the gradient (the
    selection is computed without one), Adam from the formula."""
    ps = [torch.tensor(t).requires_grad_() for wb in ts["online"] for t in wb]
    tg = [torch.tensor(t) for wb in ts["target"] for t in wb]
    q = _torch_forward(ps, torch.tensor(X))
    qa = q.gather(1, torch.tensor(act, dtype=torch.long)[:, None])[:, 0]
    with torch.no_grad():
        sel = _torch_forward(ps, torch.tensor(Xn)).argmax(dim=1)
        nxt = _torch_forward(tg, torch.tensor(Xn)).gather(1, sel[:, None])[:, 0]
        td = torch.tensor(rew) + hp.gamma * nxt * (1 - torch.tensor(done, dtype=torch.float32))
    loss = ((qa - td) ** 2).mean()
    loss.backward()
    ts["t"] += 1
    t = ts["t"]
    new_p, new_m, new_v = [], [], []
    for p, m, v in zip(ps, [x for wb in ts["m"] for x in wb], [x for wb in ts["v"] for x in wb]):
        g = p.grad
        m = (1 - hp.beta1) * g + hp.beta1 * torch.tensor(m)
        v = (1 - hp.beta2) * g * g + hp.beta2 * torch.tensor(v)
        u = (m / (1 - hp.beta1 ** t)) / (torch.sqrt(v / (1 - hp.beta2 ** t)) + hp.adam_eps)
        new_p.append((p.detach() - hp.learning_rate * u).numpy())
        new_m.append(m.numpy())
        new_v.append(v.numpy())
    pair = lambda xs: [(xs[i], xs[i + 1]) for i in range(0, len(xs), 2)]  # noqa: E731
    ts["online"], ts["m"], ts["v"] = pair(new_p), pair(new_m), pair(new_v)
    return float(loss.detach())


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / (1e-3 + np.max(np.abs(b))))


def test_reference_with_double_on_matches_a_torch_restatement():
    """double_step(double=True) against autograd on the Double DQN loss with
    Adam from the formula, both run five steps from the same start without
    resynchronising: every parameter (online, target, both moments) agrees
    within REL_TOL after each step, the fifth included, and the losses too.
    The two sides select with their own qs."""
    ring = host_ring("f32")
    hp = ohp(8)
    online, target = host_nets(150, (16, 16), 5)
    st = O.LearnerState.start(online, target, 1.0)
    ts = {"online": [(w.copy(), b.copy()) for w, b in online], "target": [(w.copy(), b.copy()) for w, b in target],
          "m": [(np.zeros_like(w), np.zeros_like(b)) for w, b in online],
          "v": [(np.zeros_like(w), np.zeros_like(b)) for w, b in online], "t": 0}
    for step in range(5):
        info = D.double_step(st, hp, *_ring_args(ring), CAP)
        idx = info["rows"]
        loss = _torch_double_step(ts, hp, ring["obs"][idx], ring["next_obs"][idx], ring["actions"][idx],
                                  ring["rewards"][idx], ring["dones"][idx])
        assert abs(float(info["loss"]) - loss) <= REL_TOL * (1e-3 + abs(loss)), step
        if step % hp.target_update_interval == 0:
            ts["target"] = [(F(hp.tau) * w + F(1 - hp.tau) * tw, F(hp.tau) * b + F(1 - hp.tau) * tb)
                            for (w, b), (tw, tb) in zip(ts["online"], ts["target"])]
        for k in SETS:
            for (a, b), (c, d) in zip(getattr(st, k), ts[k]):
                assert _rel(a, c) <= REL_TOL and _rel(b, d) <= REL_TOL, (step, k)


DISCRIMINATING = [(kind, net, A) for kind in ("f32", "code") for net in NETS for A in (5, 8)] + \
    [("code", "wide", 5)]


@pytest.mark.parametrize("kind,net,A", DISCRIMINATING, ids=[f"{k}-{n}-a{a}" for k, n, a in DISCRIMINATING])
def test_reference_data_discriminates_the_two_rules(kind, net, A):
    """On the reference alone, for every net and ring the GPU tests use: of
    the first step's 65 rows at least a quarter select another action than
    the target net's own maximum (argmax qs != argmax qt) AND thereby take
    another value (qt[a*] != max qt).  Independently initialised nets give
    this a wide margin (0.57 to 0.79 measured for these widths)."""
    ring = host_ring(kind)
    hidden = (256, 128, 64) if net == "wide" else NETS[net]
    online, target = host_nets(ring["n_in"], hidden, A)
    st = O.LearnerState.start(online, target, 1.0)
    info = D.double_step(st, ohp(65), *_ring_args(ring), CAP, code_window=ring["window"])
    qs, qt, sel = info["qs"], info["qt"], info["sel"]
    differs = [(sel[b] != int(np.argmax(qt[b]))) and (qt[b, sel[b]] != qt[b].max()) for b in range(65)]
    assert sum(differs) >= 65 / 4, sum(differs) / 65
    assert all(sel[b] == int(np.argmax(qs[b])) for b in range(65))  # (the first maximum: numpy's argmax rule too)


def test_selection_takes_the_first_maximum_and_no_nan():
    assert D.select(np.array([1, 3, 3, 2], F)) == 1
    assert D.select(np.array([2, 2, 2], F)) == 0
    assert D.select(np.array([np.nan, 5, 1], F)) == 0  # (nothing compares greater than a NaN)
    assert D.select(np.array([1, np.nan, 5], F)) == 2


def _desc(in_features, hidden, inp=0, precision=1, n_actions=5):
    from dronerl_amd.dqn import DrlQnetDesc
    h = list(hidden) + [0] * (3 - len(hidden))
    return DrlQnetDesc(in_features, len(hidden), (ctypes.c_int32 * 3)(*h), n_actions, precision, inp)


def _wdesc(in_features, hidden, inp=0, n_actions=5):
    from dronerl_amd.dqn import DrlWidenetDesc
    h = list(hidden) + [0] * (3 - len(hidden))
    return DrlWidenetDesc(in_features, len(hidden), (ctypes.c_int32 * 3)(*h), n_actions, inp)


def test_double_calls_validate_as_the_max_rule_calls_do():
    """Every pointer, alignment, batch, size and row kind is checked before
    any device work (no GPU needed), and each refusal carries the message of
    the corresponding max-rule call: NULL and misaligned arguments, batch 0
    and 4097, a code-row mismatch."""
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import DQNHParams, DrlPerHParams, DrlReplay, _bind, _bind_widenet
    L = _bind_widenet(_bind(lib()))
    vp = ctypes.c_void_p
    hp = DQNHParams(batch=64).c()
    ph = DrlPerHParams(0.6, 0.4, 0, 1e-6)
    good = DrlReplay(5000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    pairs = [("drl_dqn_large_train", "drl_dqn_double_train", _desc, False),
             ("drl_widenet_dqn_train", "drl_widenet_dqn_double_train", _wdesc, False),
             ("drl_dqn_per_train", "drl_dqn_double_per_train", _desc, True),
             ("drl_widenet_dqn_per_train", "drl_widenet_dqn_double_per_train", _wdesc, True)]
    cases = [dict(h=None), dict(agent=None), dict(agent=vp((1 << 20) + 8)), dict(packed=None),
             dict(packed=vp((1 << 21) + 4)), dict(r=None),
             dict(r=DrlReplay(5000, 294, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)),
             dict(r=DrlReplay(0, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)), dict(size=-1), dict(size=5001),
             dict(r=DrlReplay(5000, 292, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)), dict(code=True),
             dict(r=DrlReplay(5000, 294, (1 << 20) + 2, 1 << 20, 1 << 20, 1 << 20, 1 << 20)),
             dict(h=DQNHParams(batch=0).c()), dict(h=DQNHParams(batch=4097).c()),
             dict(h=DQNHParams(batch=64, target_update_interval=0).c()), dict(h=DQNHParams(batch=64, beta1=1.0).c()),
             dict(desc=None)]
    per_cases = [dict(per=None), dict(per=vp((1 << 22) + 8)), dict(ph=None)]  # (every case is refused: nothing launches)
    for base, dbl, mk, is_per in pairs:
        def call(name, desc="d", h=hp, agent=vp(1 << 20), packed=vp(1 << 21), r=good, size=100, code=False,
                 per=vp(1 << 22), ph=ph):
            d = None if desc is None else mk(294, (128, 64), 1 if code else 0)
            args = [None if d is None else ctypes.byref(d), None if h is None else ctypes.byref(h)]
            if is_per:
                args.append(None if ph is None else ctypes.byref(ph))
            args += [agent, packed, None if r is None else ctypes.byref(r), size]
            if is_per:
                args.append(per)
            rc = getattr(L, name)(*args, None)
            return rc, L.drl_last_error()
        for kw in cases + (per_cases if is_per else []):
            want, got = call(base, **kw), call(dbl, **kw)
            assert want[0] != 0 and got[0] != 0 and want[1] == got[1] and got[1], (dbl, kw, want, got)


def test_double_refusals_and_cli(monkeypatch):
    """DQNHParams.double_dqn is the last field and leaves c() alone;
    make_learner sends a QNetwork with it to the chain at every batch; every
    learner without a Double chain refuses by a named constant at
    construction (before any device work); the drivers parse or refuse
    --double_dqn by name; the sweep's grid takes JSON booleans."""
    import dataclasses

    from dronerl_amd import dqn, global_learner, league, population, selfplay, sweep, train
    hp = dqn.DQNHParams(double_dqn=True)
    assert [f.name for f in dataclasses.fields(dqn.DQNHParams)][-1] == "double_dqn" and not dqn.DQNHParams().double_dqn
    assert bytes(hp.c()) == bytes(dqn.DQNHParams().c())
    made = []
    for name in ("DQNLearner", "LargeBatchDQNLearner"):
        monkeypatch.setattr(dqn, name, lambda net, hp, _n=name, **kw: made.append(_n) or _n)
    for batch in (1, 8, 64, 65, 4096):
        assert dqn.make_learner(object(), dqn.DQNHParams(batch=batch, double_dqn=True)) == "LargeBatchDQNLearner"
    assert dqn.make_learner(object(), dqn.DQNHParams(batch=8)) == "DQNLearner"
    monkeypatch.undo()

    class Net:  # (the refusals come before anything reads the net)
        L = device = None
    for cls, msg in ((dqn.DQNLearner, dqn.DOUBLE_SINGLE_LAUNCH_REFUSAL), (dqn.ConvDQNLearner, dqn.DOUBLE_CONV_REFUSAL),
                     (dqn.LargeBatchConvDQNLearner, dqn.DOUBLE_CONV_REFUSAL),
                     (dqn.PrioritizedConvDQNLearner, dqn.DOUBLE_CONV_REFUSAL)):
        with pytest.raises(ValueError, match=re.escape(msg)):
            cls(Net(), hp)
    hps = [dqn.DQNHParams(), hp]
    for make, msg in ((lambda: population.ConvPopulationDQN((7, 7, 6), (), (16,), hps, 4),
                       population.DOUBLE_CONV_POP_REFUSAL),
                      (lambda: population.PrioritizedPopulationDQN(294, (16, 16), hps, 4),
                       population.DOUBLE_PER_POP_REFUSAL),
                      (lambda: league.LeagueDQN(294, (16, 16), hps, 4), league.DOUBLE_LEAGUE_REFUSAL),
                      (lambda: league.ConvLeagueDQN((7, 7, 6), (), (16,), hps, 4), league.DOUBLE_LEAGUE_REFUSAL),
                      (lambda: selfplay.SelfPlayDQN(294, (16, 16), hps, 4), selfplay.DOUBLE_SELFPLAY_REFUSAL),
                      (lambda: selfplay.ConvSelfPlayDQN((7, 7, 6), (), (16,), hps, 4),
                       selfplay.DOUBLE_SELFPLAY_REFUSAL)):
        with pytest.raises(ValueError, match=re.escape(msg)):
            make()
    assert "double_dqn" in global_learner.DOUBLE_SHARDED_REFUSAL
    # the drivers
    a = train.parse_args(["--double_dqn"])
    assert a.double_dqn and train.hparams_of(a).double_dqn and not train.hparams_of(train.parse_args([])).double_dqn
    assert train.parse_args(["--double_dqn", "--hidden_layers", "256", "128", "64"]).double_dqn
    assert train.parse_args(["--double_dqn", "--prioritized_replay"]).double_dqn
    with pytest.raises(ValueError, match=re.escape(train.DOUBLE_CONV_REFUSAL)):
        train.parse_args(["--double_dqn", "--network_type", "conv"])
    with pytest.raises(ValueError, match=re.escape(train.DOUBLE_SHARDING_REFUSAL)):
        train.parse_args(["--double_dqn", "--use_sharding", "--num_envs", "4"])
    from dronerl_amd import conv_league, conv_selfplay, conv_sweep, per_sweep, per_train
    assert per_train.parse_args(["--double_dqn"]).double_dqn
    assert per_train.parse_args(["--double_dqn", "--hidden_layers", "256", "128", "64"]).double_dqn
    with pytest.raises(ValueError, match="--double_dqn"):
        per_train.parse_args(["--double_dqn", "--network_type", "conv"])
    for mod in (per_sweep, conv_sweep, league, conv_league, selfplay, conv_selfplay):
        with pytest.raises(ValueError, match="--double_dqn"):
            mod.parse_args(["--double_dqn"])
        with pytest.raises(ValueError, match="double_dqn"):
            mod.parse_args(["--grid", '{"double_dqn": [true]}'])
    assert "double_dqn" in sweep.MEMBER_OPTIONS
    args, points = sweep.parse_args(["--grid", '{"double_dqn": [false, true]}', "--members_seeds", "2"])
    hps, seeds, rows = sweep.members_of(args, points)
    assert [h.double_dqn for h in hps] == [False, False, True, True] and [r["double_dqn"] for r in rows] == \
        [False, False, True, True]
    with pytest.raises(ValueError, match="JSON booleans"):
        sweep.parse_args(["--grid", '{"double_dqn": [0, 1]}'])


# Every __global__ kernel under csrc/doubledqn/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_dqn_double_forward_kernel": "test_double_dqn.py::test_double_step_matches_reference_bit_exact",
    "drl_dqn_double_td_kernel": "test_double_dqn.py::test_double_step_matches_reference_bit_exact",
    "drl_dqn_double_per_td_kernel": "test_double_dqn.py::test_double_prioritized_matches_reference",
    "drl_pop_double_forward_kernel": "test_population_double.py::test_population_members_choose_their_rule",
    "drl_pop_double_td_kernel": "test_population_double.py::test_population_members_choose_their_rule",
}


def test_every_doubledqn_kernel_has_a_gpu_test():
    import glob
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "doubledqn", "*.hip")):
        src = open(f).read()
        for m in re.finditer(r"__global__", src):
            k = re.search(r"\b(drl_[a-z0-9_]+_kernel)\s*\(", src[m.end():m.end() + 300])
            if k:
                found.add(k.group(1))
    assert found == set(KERNEL_TESTS), (sorted(found - set(KERNEL_TESTS)), sorted(set(KERNEL_TESTS) - found))
    for kern, ref in KERNEL_TESTS.items():
        fname, test = ref.split("::")
        text = open(os.path.join(HERE, fname)).read()
        assert re.search(rf"^@gpu\n(?:@pytest[^\n]*\n)*def {test}\(", text, re.M), (kern, ref)


# ------------------------------------------------------------------- GPU ---
def _host(t):
    return t.detach().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def dev_ring(kind):
    """host_ring on the device: a full dqn.ReplayBuffer (shared, read only)."""
    from dronerl_amd.dqn import ReplayBuffer
    h = host_ring(kind)
    rb = ReplayBuffer(CAP, h["n_in"], torch.device("cuda"), code_radius=3 if kind == "code" else 0)
    rb.obs.copy_(torch.from_numpy(h["obs"]).reshape(rb.obs.shape))
    rb.next_obs.copy_(torch.from_numpy(h["next_obs"]).reshape(rb.next_obs.shape))
    rb.actions.copy_(torch.from_numpy(h["actions"]))
    rb.rewards.copy_(torch.from_numpy(h["rewards"]))
    rb.dones.copy_(torch.from_numpy(h["dones"]))
    rb.size, rb.cursor = CAP, 0
    torch.cuda.synchronize()
    return rb


def make(kind, hidden, A, batch, double=True, cls=None, wide=False, nets=None, **kw):
    """(net, learner, reference state, oracle hparams, hparams) on `kind`'s
    ring from host_nets' parameters."""
    from dronerl_amd import dqn
    h = host_ring(kind)
    online, target = nets or host_nets(h["n_in"], hidden, A)
    inp = "code" if kind == "code" else "obs"
    if wide:
        net = dqn.WideQNetwork(h["n_in"], hidden, n_actions=A, input=inp)
    else:
        net = dqn.QNetwork(h["n_in"], hidden, n_actions=A, precision="f32", input=inp)
    net.load([torch.from_numpy(w) for w, _ in online], [torch.from_numpy(b) for _, b in online])
    hp = dqn.DQNHParams(batch=batch, double_dqn=double, **{**STEP_KW, **kw})
    cls = cls or (dqn.WideDQNLearner if wide else dqn.LargeBatchDQNLearner)
    learner = cls(net, hp, target=([torch.from_numpy(w) for w, _ in target], [torch.from_numpy(b) for _, b in target]))
    st = O.LearnerState.start(online, target, 1.0)
    return net, learner, st, ohp(batch, **kw), hp


def ref_counters(st):
    return {"step": st.step, "count": st.count, "epsilon": float(st.epsilon), "loss": float(st.loss),
            "beta1_pow": st.beta1_pow, "beta2_pow": st.beta2_pow}


def assert_same(learner, st, where):
    for k in SETS:
        for l, ((w, b), (ow, ob)) in enumerate(zip(learner.params(k), getattr(st, k))):
            assert np.array_equal(_host(w).view(np.int32), ow.view(np.int32)), (where, k, l, "W")
            assert np.array_equal(_host(b).view(np.int32), ob.view(np.int32)), (where, k, l, "b")
    assert learner.counters() == ref_counters(st), where


def assert_packed_is_fresh(net):
    after = net.packed.clone()
    net.pack()
    torch.cuda.synchronize()
    assert torch.equal(after, net.packed)


@gpu
@pytest.mark.parametrize("A", [5, 8], ids=["a5-head-padded-to-8", "a8"])
@pytest.mark.parametrize("kind", ["code", "f32"])
@pytest.mark.parametrize("net", list(NETS))
def test_double_step_matches_reference_bit_exact(net, kind, A):
    """drl_dqn_double_train against tests/_double_ref at batches 1, 8, 64 and
    65: eight steps with a target blend of tau 0.5 every third step, so the
    online and the target net differ throughout.  After every step the online
    and target sets, both Adam sets, the counters (as dicts) and the loss are
    equal on bits; at the end the packed image is a fresh drl_qnet_pack."""
    for batch in BATCHES:
        nn, learner, st, hp, _ = make(kind, NETS[net], A, batch)
        ring, rb = host_ring(kind), dev_ring(kind)
        for t in range(8):
            D.double_step(st, hp, *_ring_args(ring), CAP, code_window=ring["window"])
            learner.train(rb)
            torch.cuda.synchronize()
            assert_same(learner, st, (batch, t))
        assert learner.counters()["count"] == 8
        learner.check_errors()
        assert_packed_is_fresh(nn)


@gpu
def test_double_differs_from_max_rule_on_the_same_rows():
    """The same start and rows under drl_dqn_large_train end with other online
    bits after one step, and the max-rule learner equals the reference with
    double=False: the two entry points run two rules."""
    ring, rb = host_ring("code"), dev_ring("code")
    _, dbl, st_d, hp, _ = make("code", (16, 16), 5, 64)
    _, mx, st_m, _, _ = make("code", (16, 16), 5, 64, double=False)
    assert torch.equal(dbl.sets["online"].view(torch.int32), mx.sets["online"].view(torch.int32))
    dbl.train(rb)
    mx.train(rb)
    torch.cuda.synchronize()
    D.double_step(st_d, hp, *_ring_args(ring), CAP, code_window=7)
    D.double_step(st_m, hp, *_ring_args(ring), CAP, code_window=7, double=False)
    assert_same(dbl, st_d, "double")
    assert_same(mx, st_m, "max")
    assert not torch.equal(dbl.sets["online"].view(torch.int32), mx.sets["online"].view(torch.int32))
    assert dbl.counters()["loss"] != mx.counters()["loss"]


@gpu
def test_double_equals_max_rule_when_target_is_online():
    """target= the online weights, tau 1, interval 1: the target set equals
    the online set whenever a step starts, so qs == qt and six Double steps
    are LargeBatchDQNLearner's bit for bit (sets, counters, packed image)."""
    rb = dev_ring("code")
    online, _ = host_nets(294, (24, 16, 8), 5)
    kw = dict(nets=(online, online), tau=1.0, target_update_interval=1)
    net_d, dbl, _, _, _ = make("code", (24, 16, 8), 5, 65, **kw)
    net_m, mx, _, _, _ = make("code", (24, 16, 8), 5, 65, double=False, **kw)
    for t in range(6):
        dbl.train(rb)
        mx.train(rb)
        torch.cuda.synchronize()
        for k in SETS:
            assert torch.equal(dbl.sets[k].view(torch.int32), mx.sets[k].view(torch.int32)), (t, k)
        assert dbl.counters() == mx.counters() and dbl.counters()["loss"] > 0, t
        assert torch.equal(net_d.packed, net_m.packed), t


@gpu
def test_double_tie_and_selection_by_hand():
    """Net (8,): an online Q head of zero weights and equal biases makes qs
    all equal, so a* = 0 (the lowest index); the target's head of zero
    weights and biases [1, 5, 2, 3, 4] makes qt those biases.  The loss is
    the hand-computed mean of (0.25 - (r + gamma * 1 * (1 - done)))^2 over
    the step's rows, exactly; the max-rule call gives the value with 5."""
    ring, rb = host_ring("f32"), dev_ring("f32")
    online, target = host_nets(150, (8,), 5)
    online[1] = (np.zeros_like(online[1][0]), np.full(5, 0.25, F))
    target[1] = (np.zeros_like(target[1][0]), np.array([1, 5, 2, 3, 4], F))
    rows = O.sample_indices(STEP_KW["sample_seed"], 0, 8, CAP)

    def by_hand(nxt):
        loss = F(0.0)
        for s in rows:
            notdone = F(0.0) if ring["dones"][s] else F(1.0)
            d = F(0.25) - (F(ring["rewards"][s]) + (F(0.9) * F(nxt)) * notdone)
            loss = F(loss + d * d)
        return float(F(loss / F(8)))

    for double, nxt in ((True, 1.0), (False, 5.0)):
        _, learner, _, _, _ = make("f32", (8,), 5, 8, double=double, nets=(online, target))
        learner.train(rb)
        torch.cuda.synchronize()
        assert learner.counters()["loss"] == by_hand(nxt), double
    assert by_hand(1.0) != by_hand(5.0)


@gpu
def test_double_without_a_sample_only_blends():
    """size < batch: no train step; the target blend happens when due (steps
    0 and 3), epsilon decays and the step advances, as the reference has it;
    Adam's sets and count stay put."""
    ring, rb0 = host_ring("code"), dev_ring("code")
    from dronerl_amd.dqn import ReplayBuffer
    rb = ReplayBuffer(CAP, 294, torch.device("cuda"), code_radius=3)
    for k in ("obs", "next_obs", "actions", "rewards", "dones"):
        getattr(rb, k).copy_(getattr(rb0, k))
    rb.size = 5
    _, learner, st, hp, _ = make("code", (16, 16), 5, 8)
    target0 = learner.sets["target"].clone()
    for t in range(5):
        info = D.double_step(st, hp, *_ring_args(ring), 5, code_window=7)
        assert not info["trained"]
        learner.train(rb)
        torch.cuda.synchronize()
        assert_same(learner, st, t)
    assert learner.counters()["count"] == 0 and learner.counters()["step"] == 5
    assert not torch.equal(target0, learner.sets["target"]) and not learner.sets["m"].any()


@gpu
@pytest.mark.parametrize("batch", [8, 65])
def test_double_wide_matches_reference(batch):
    """drl_widenet_dqn_double_train on net 256-128-64 (16 unit tiles in the
    first layer), three steps, bit for bit; the packed image is a fresh
    drl_widenet_pack."""
    net, learner, st, hp, _ = make("code", (256, 128, 64), 5, batch, wide=True)
    ring, rb = host_ring("code"), dev_ring("code")
    for t in range(3):
        D.double_step(st, hp, *_ring_args(ring), CAP, code_window=7)
        learner.train(rb)
        torch.cuda.synchronize()
        assert_same(learner, st, t)
    learner.check_errors()
    assert_packed_is_fresh(net)


def _per_run(hidden, batch, wide, alpha, beta0, steps):
    """The prioritized Double step against the reference on the sampler's own
    slots and weights, read back from the block after each step."""
    from dronerl_amd import dqn
    ring, rb = host_ring("code"), dev_ring("code")
    cls = dqn.PrioritizedWideDQNLearner if wide else dqn.PrioritizedDQNLearner
    net, learner, st, hp, _ = make("code", hidden, 5, batch, cls=cls, wide=wide)
    per = dqn.PrioritizedReplay(rb, alpha=alpha, beta0=beta0, beta_steps=0, eps=1e-6, batch=batch)
    P = per.layout.leaves
    for t in range(steps):
        learner.train(per)
        torch.cuda.synchronize()
        slots, w = _host(per.slots), _host(per.weights)
        if alpha == 0 and beta0 == 0:
            assert (w == 1.0).all()
            # ... and the step is the uniform Double step on the same slots
            info = D.double_step(st, hp, *_ring_args(ring), CAP, slots=slots, code_window=7)
        else:
            info = D.double_step(st, hp, *_ring_args(ring), CAP, slots=slots, weights=w, code_window=7)
        assert_same(learner, st, (t, "sets"))
        assert np.array_equal(_bits(_host(per.abs_td)), _bits(info["absd"])), t
        # the new leaves: priority32(|d|), the largest of the rows that drew the slot, within the tolerance
        # tests/test_prioritized_replay.py uses for this comparison (1 f32 ulp of the float64 formula)
        p_dev = _host(per.tree)[P + slots]
        p_ref = R.priority32(info["absd"], 1e-6, alpha)
        best = {}
        for s, p in zip(slots.tolist(), p_ref.tolist()):
            best[s] = max(best.get(s, 0.0), p)
        want = np.array([best[s] for s in slots.tolist()], F)
        assert (R.ulps(p_dev, want) <= 1).all(), t
    learner.check_errors()
    assert_packed_is_fresh(net)
    return learner


PER_CASES = {"h16-16-b8": ((16, 16), 8, False), "h128-64-b65": ((128, 64), 65, False), "wide-b65": ((256, 128, 64), 65, True)}


@gpu
@pytest.mark.parametrize("hidden,batch,wide", list(PER_CASES.values()), ids=list(PER_CASES))
def test_double_prioritized_matches_reference(hidden, batch, wide):
    """drl_dqn_double_per_train (and the wide call at one shape) with alpha
    0.6 and beta 0.4: each of four steps matches _double_ref on the sampler's
    slots and weights, |d| on bits, the new leaves priority32(|d|)."""
    learner = _per_run(hidden, batch, wide, 0.6, 0.4, 4)
    assert learner.counters()["count"] == 4


@gpu
def test_double_prioritized_alpha0_beta0_is_the_uniform_double_step():
    """alpha 0 and beta 0: every weight is exactly 1.0 and the step equals
    the unweighted Double step on the drawn slots bit for bit."""
    _per_run((16, 16), 64, False, 0.0, 0.0, 4)


def _capture_and_compare(make_pair, train, steps=5):
    (net_e, eager, arg_e), (net_g, graphed, arg_g) = make_pair(), make_pair()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            train(graphed, arg_g)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert graphed.counters()["step"] == 0  # (capturing runs nothing)
    for _ in range(steps):
        g.replay()
        train(eager, arg_e)
    torch.cuda.synchronize()
    assert eager.counters()["step"] == steps and eager.counters()["count"] == steps
    for k in SETS:
        assert torch.equal(eager.sets[k].view(torch.int32), graphed.sets[k].view(torch.int32)), k
    assert eager.counters() == graphed.counters()
    assert torch.equal(net_e.packed, net_g.packed)
    return arg_e, arg_g


@gpu
@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_double_learner_is_graph_capturable(prioritized):
    """One Double train() captured with torch.cuda.graph and replayed 5 times
    equals 5 eager calls on a twin bit for bit (sets, counters, packed image,
    and the prioritized block): kernel nodes only, and the step, Adam's count
    and the row draw live on the device."""
    from dronerl_amd import dqn
    rb = dev_ring("code")

    def make_pair():
        cls = dqn.PrioritizedDQNLearner if prioritized else None
        net, learner, _, _, _ = make("code", (128, 64), 5, 65, cls=cls)
        arg = dqn.PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=4, batch=65) if prioritized else rb
        return net, learner, arg

    arg_e, arg_g = _capture_and_compare(make_pair, lambda learner, arg: learner.train(arg))
    if prioritized:
        assert torch.equal(arg_e.block, arg_g.block)


@gpu
def test_refused_double_calls_move_no_counter():
    """A refused call returns before any device work: the counters stay."""
    from dronerl_amd._native import DroneRLError
    rb = dev_ring("f32")  # (f32 rows for a code net: the row-kind mismatch)
    _, learner, _, _, _ = make("code", (16, 16), 5, 8)
    before = learner.counters()
    with pytest.raises(DroneRLError, match="policy codes"):
        learner.train(rb)
    torch.cuda.synchronize()
    assert learner.counters() == before and before["step"] == 0


@gpu
def test_train_cli_double_dqn_runs():
    """train(..., double_dqn=True): 64 envs, 30 steps, net 16-16 at the
    default batch 8 -- make_learner picked the launch chain (the single-launch
    learner has no selector); the run finishes with a finite loss and a
    finite greedy eval."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import LargeBatchDQNLearner, QNetwork
    from dronerl_amd.train import evaluate, train
    params = EnvParams(n_drones=4, grid_size=9)
    res = train(params, 64, 30, hidden=(16, 16), double_dqn=True, memory_size=2000)
    assert isinstance(res.learner, LargeBatchDQNLearner) and res.learner.hp.double_dqn and res.learner.hp.batch == 8
    c = res.learner.counters()
    assert c["step"] == 30 and c["count"] == 30 and np.isfinite(c["loss"])
    qnet = QNetwork(res.net.in_features, res.net.hidden, precision="f32")  # (the eval's act reads f32 rows)
    qnet.load(*zip(*res.learner.params("online")))
    (mean, std), _, _ = evaluate(params, qnet, num_evals=2, num_eval_steps=200)
    assert np.isfinite(mean) and np.isfinite(std)
