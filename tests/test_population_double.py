"""Double DQN targets chosen per member of a dense population:
drl_pop_double_train (dronerl_amd/csrc/doubledqn/), PopulationDQN's
`double_mask`, and the sweep's per-member "double_dqn" option.

A member whose byte is 0 is the max-rule member of drl_pop_train bit for bit;
a member whose byte is set is a single drl_widenet_dqn_double_train agent with
its hyperparameters on its ring bit for bit (that call is pinned against
tests/_double_ref in tests/test_double_dqn.py); neither depends on what its
neighbours chose.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_double_dqn import CAP, host_nets, host_ring

gpu = pytest.mark.gpu
F = np.float32
SETS = ("online", "target", "m", "v")
HIDDEN, BATCHES, MAX_BATCH = (16, 16), (8, 8, 16), 16
SIZES = (10, 12, 14, 16, 18, 20)  # the rings' size at the six steps: member 2 (batch 16) only blends for three


def _hps(mask):
    from dronerl_amd.dqn import DQNHParams
    return [DQNHParams(batch=b, double_dqn=bool(d), tau=0.5, target_update_interval=3, sample_seed=20 + m,
                       learning_rate=1e-3 * (m + 1), epsilon_decay=0.95, epsilon_decay_every=2)
            for m, (b, d) in enumerate(zip(BATCHES, mask))]


def _member_ring(m):
    """Member m's ring on the host: the shared code ring's rows rotated by 37 m
    (another ring per member from one fixture)."""
    h = host_ring("code")
    return {k: np.roll(h[k], 37 * m, axis=0) for k in ("obs", "next_obs", "actions", "rewards", "dones")}


def _pop(mask):
    """(population, replay): three members on 16-16 from host_nets' parameters
    (seed m), their rings prefilled; the caller sets replay.size."""
    from dronerl_amd.population import PopulationDQN, PopulationReplay
    nets = [host_nets(294, HIDDEN, 5, seed=m) for m in range(3)]
    tens = lambda ps: ([torch.from_numpy(w) for w, _ in ps], [torch.from_numpy(b) for _, b in ps])  # noqa: E731
    pop = PopulationDQN(294, HIDDEN, _hps(mask), 4, online=[tens(o) for o, _ in nets], target=[tens(t) for _, t in nets],
                        max_batch=MAX_BATCH)
    rb = PopulationReplay(3, CAP, 3)
    for m in range(3):
        ring, views = _member_ring(m), rb.ring(m)
        for k in views:
            views[k].copy_(torch.from_numpy(ring[k]).reshape(views[k].shape))
    torch.cuda.synchronize()
    return pop, rb


def _single(m, double):
    """Member m as one agent: drl_widenet_dqn(_double)_train on its ring."""
    from dronerl_amd import dqn
    online, target = host_nets(294, HIDDEN, 5, seed=m)
    net = dqn.WideQNetwork(294, HIDDEN, n_actions=5, input="code")
    net.load([torch.from_numpy(w) for w, _ in online], [torch.from_numpy(b) for _, b in online])
    mask = [0, 0, 0]
    mask[m] = int(double)
    learner = dqn.WideDQNLearner(net, _hps(mask)[m], target=([torch.from_numpy(w) for w, _ in target],
                                                            [torch.from_numpy(b) for _, b in target]))
    rb = dqn.ReplayBuffer(CAP, 294, torch.device("cuda"), code_radius=3)
    ring = _member_ring(m)
    for k, v in ring.items():
        getattr(rb, k).copy_(torch.from_numpy(v).reshape(getattr(rb, k).shape))
    return learner, rb


def _assert_member_is(pop, m, learner, where):
    for k in SETS:
        for l, ((w, b), (sw, sb)) in enumerate(zip(pop.params(k, m), learner.params(k))):
            assert torch.equal(w.view(torch.int32), sw.view(torch.int32)), (where, m, k, l, "W")
            assert torch.equal(b.view(torch.int32), sb.view(torch.int32)), (where, m, k, l, "b")
    c = pop.counters(m)
    c.pop("trained")
    assert c == learner.counters(), (where, m)


# ------------------------------------------------------------------- CPU ---
def test_pop_double_train_validates_as_pop_train_does():
    """Every argument is checked before any device work (no GPU needed) with
    drl_pop_train's checks and messages; d_double must be non-NULL."""
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import DrlReplay, _bind
    from dronerl_amd.population import _bind_pop, pop_desc
    L = _bind_pop(_bind(lib()))
    vp = ctypes.c_void_p
    good = DrlReplay(500, 32, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def call(name, desc=pop_desc(294, (16, 16)), members=3, max_batch=16, d_pop=vp(1 << 20), r=good, size=100):
        args = [None if desc is None else ctypes.byref(desc), members, max_batch, d_pop,
                None if r is None else ctypes.byref(r), size]
        if name == "drl_pop_double_train":
            args.append(vp(1 << 22))
        return getattr(L, name)(*args, None), L.drl_last_error()

    cases = [dict(desc=None), dict(desc=pop_desc(294, (12,))), dict(members=0), dict(members=1025), dict(max_batch=0),
             dict(max_batch=4097), dict(d_pop=None), dict(d_pop=vp((1 << 20) + 8)), dict(r=None),
             dict(r=DrlReplay(500, 32, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)),
             dict(r=DrlReplay(0, 32, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)),
             dict(r=DrlReplay(500, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)),  # (f32 rows: a code-row mismatch)
             dict(r=DrlReplay(500, 32, (1 << 20) + 2, 1 << 20, 1 << 20, 1 << 20, 1 << 20)), dict(size=-1), dict(size=501)]
    for kw in cases:
        want, got = call("drl_pop_train", **kw), call("drl_pop_double_train", **kw)
        assert want[0] == -1 and got[0] == -1 and want[1] == got[1] and got[1], (kw, want, got)
    d = pop_desc(294, (16, 16))
    assert L.drl_pop_double_train(ctypes.byref(d), 3, 16, vp(1 << 20), ctypes.byref(good), 100, None, None) == -1
    assert b"d_double is NULL" in L.drl_last_error()


# ------------------------------------------------------------------- GPU ---
@gpu
def test_population_members_choose_their_rule():
    """Mask [0, 1, 1], batches [8, 8, 16], max_batch 16, six steps on rings
    growing from 10 rows: members 0 and 1 train from the start, member 2 only
    blends until its ring holds 16.  After every step member 0's whole block
    equals the same member's under drl_pop_train, and members 1 and 2 equal
    single drl_widenet_dqn_double_train agents (sets and counters on bits)."""
    pop, rb = _pop([0, 1, 1])
    ref, rb_ref = _pop([0, 0, 0])
    assert pop.double_mask.tolist() == [0, 1, 1] and pop._any_double and not ref._any_double
    singles = {m: _single(m, True) for m in (1, 2)}
    max_single = _single(1, False)
    for t, size in enumerate(SIZES):
        rb.size = rb_ref.size = size
        pop.train(rb)
        ref.train(rb_ref)
        for learner, ring in (*singles.values(), max_single):
            ring.size = size
            learner.train(ring)
        torch.cuda.synchronize()
        assert torch.equal(pop.member_block(0), ref.member_block(0)), t
        for m, (learner, _) in singles.items():
            _assert_member_is(pop, m, learner, t)
        assert pop.counters(2)["count"] == max(0, t - 2) and pop.counters(1)["count"] == t + 1
    # ... and the rule mattered: member 1 under the max rule ended elsewhere
    assert not torch.equal(pop.params("online", 1)[0][0], max_single[0].params("online")[0][0])
    _assert_member_is(ref, 1, max_single[0], "max")


@gpu
def test_all_zero_mask_is_drl_pop_train_byte_for_byte():
    """drl_pop_double_train with every byte 0 leaves the whole population
    block (parameters, counters, scratch, records) as drl_pop_train does."""
    from dronerl_amd.dqn import _check, _stream, _vp
    a, rb_a = _pop([0, 0, 0])
    b, rb_b = _pop([0, 0, 0])
    zeros = torch.zeros(3, dtype=torch.uint8, device="cuda")
    for size in SIZES:
        rb_a.size = rb_b.size = size
        _check(a.L, a.L.drl_pop_double_train(ctypes.byref(a.desc), 3, MAX_BATCH, _vp(a.block.data_ptr()),
                                             ctypes.byref(rb_a._c), size, _vp(zeros.data_ptr()), _stream(a.device)))
        b.train(rb_b)
    torch.cuda.synchronize()
    assert torch.equal(a.block, b.block) and a.counters(0)["count"] == 6 and a.counters(2)["count"] == 3


@gpu
def test_a_member_does_not_depend_on_its_neighbours_rule():
    """Masks [1, 1, 0] and [0, 1, 1]: member 1's block is the same."""
    a, rb_a = _pop([1, 1, 0])
    b, rb_b = _pop([0, 1, 1])
    for size in SIZES:
        rb_a.size = rb_b.size = size
        a.train(rb_a)
        b.train(rb_b)
    torch.cuda.synchronize()
    assert torch.equal(a.member_block(1), b.member_block(1))
    assert not torch.equal(a.member_block(0), b.member_block(0))


@gpu
def test_population_double_step_is_graph_capturable():
    """P = 3, mask [0, 1, 1]: one captured train() replayed 5 times equals 5
    eager calls on a twin, the whole block byte for byte."""
    (eager, rb_e), (graphed, rb_g) = _pop([0, 1, 1]), _pop([0, 1, 1])
    rb_e.size = rb_g.size = 20
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed.train(rb_g)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert graphed.counters(1)["step"] == 0  # (capturing runs nothing)
    for _ in range(5):
        g.replay()
        eager.train(rb_e)
    torch.cuda.synchronize()
    assert torch.equal(eager.block, graphed.block)
    assert [eager.counters(m)["count"] for m in range(3)] == [5, 5, 5]


@gpu
def test_population_without_a_double_member_calls_pop_train(monkeypatch):
    """PopulationDQN with no double member still calls drl_pop_train; with one
    it calls drl_pop_double_train (a spy on the bound functions)."""
    calls = []
    plain, rb = _pop([0, 0, 0])
    mixed, rb2 = _pop([0, 1, 0])
    rb.size = rb2.size = 20
    for name in ("drl_pop_train", "drl_pop_double_train"):
        real = getattr(plain.L, name)
        monkeypatch.setattr(plain.L, name, lambda *a, _n=name, _f=real: calls.append(_n) or _f(*a))
    plain.train(rb)
    assert calls == ["drl_pop_train"]
    mixed.train(rb2)
    assert calls == ["drl_pop_train", "drl_pop_double_train"]
    torch.cuda.synchronize()
    assert plain.counters(0)["count"] == 1 and mixed.counters(1)["count"] == 1
