"""The dense nets' DQN learner at replay batches up to 4096: drl_dqn_large_*
(dronerl_amd/csrc/largelearn/), dqn.LargeBatchDQNLearner, dqn.make_learner and
`python -m dronerl_amd.train --batch_size N`.

Reference: train_jax.py:68-98 (the scan body's learner block; its README
raises the batch size with the number of envs), jax_impl/agents/dqn.py:147-200,
jax_impl/buffers.py:79-93.

Oracle: oracle/dqn_learner.py, the numpy restatement of drl_dqn_train's fixed
arithmetic order, which holds for any batch: the launch chain must equal it
BIT FOR BIT (all four parameter sets, the loss, every counter, both beta
powers) after every step, and, because both learners draw their rows with the
same counter hash, equal drl_dqn_train itself at batches it takes."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import dqn_learner as O

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SETS = ("online", "target", "m", "v")


# ------------------------------------------------------------ C ABI (CPU) ---
def _desc(in_features, hidden, inp=0, precision=1, n_actions=5):
    from dronerl_amd.dqn import DrlQnetDesc
    h = list(hidden) + [0] * (3 - len(hidden))
    return DrlQnetDesc(in_features, len(hidden), (ctypes.c_int32 * 3)(*h), n_actions, precision, inp)


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind
    return _bind(lib())


def test_large_layout_query():
    """Host only: the parameter-set offsets are drl_dqn_layout_query's at the
    batches both take; the marks are disjoint and 16-byte aligned and the
    scratch grows with the batch; batches 0 and 4097 are refused by name."""
    from dronerl_amd.dqn import DrlDqnLayout
    L = _lib()
    shared = ("n_params", "online_off", "target_off", "m_off", "v_off", "counters_off", "scratch_off")
    for d in (_desc(294, (128, 64), 1), _desc(294, (16, 16), 1), _desc(150, (64,)), _desc(512, (64,), 0, 0, 8)):
        for batch in (1, 8, 64):
            a, b = DrlDqnLayout(), DrlDqnLayout()
            assert L.drl_dqn_layout_query(ctypes.byref(d), batch, ctypes.byref(a)) == 0, L.drl_last_error()
            assert L.drl_dqn_large_layout_query(ctypes.byref(d), batch, ctypes.byref(b)) == 0, L.drl_last_error()
            for k in shared:
                assert getattr(a, k) == getattr(b, k), k
            assert list(a.weight_off) == list(b.weight_off) and list(a.bias_off) == list(b.bias_off)
            assert b.grad_workgroups == 0 and b.grad_lds_bytes == 0
        last = 0
        for batch in (65, 257, 4096):
            lay = DrlDqnLayout()
            assert L.drl_dqn_large_layout_query(ctypes.byref(d), batch, ctypes.byref(lay)) == 0, L.drl_last_error()
            marks = [lay.online_off, lay.target_off, lay.m_off, lay.v_off, lay.counters_off, lay.scratch_off, lay.bytes]
            # the scratch holds at least both nets' decoded inputs and the rows' action, reward and done
            need = [4 * lay.n_params] * 4 + [64, 4 * batch * (2 * d.in_features + 3)]
            assert marks[0] == 0 and all(m % 16 == 0 for m in marks)
            assert all(marks[i] + need[i] <= marks[i + 1] for i in range(6))
            assert lay.bytes > last
            last = lay.bytes
    lay = DrlDqnLayout()
    d = _desc(294, (128, 64), 1)
    for batch in (0, 4097, -1):
        assert L.drl_dqn_large_layout_query(ctypes.byref(d), batch, ctypes.byref(lay)) != 0
        assert b"batch must be in [1, 4096]" in L.drl_last_error()
    assert L.drl_dqn_large_layout_query(None, 8, ctypes.byref(lay)) != 0 and b"NULL" in L.drl_last_error()
    assert L.drl_dqn_large_layout_query(ctypes.byref(d), 8, None) != 0 and b"layout is NULL" in L.drl_last_error()
    assert L.drl_dqn_large_layout_query(ctypes.byref(_desc(294, (136,))), 8, ctypes.byref(lay)) != 0
    assert b"hidden widths" in L.drl_last_error()


def test_large_calls_validate_before_device_work():
    """Every pointer, the alignment, the batch, the size and the row kind are
    checked before any device work (no GPU needed)."""
    from dronerl_amd.dqn import DQNHParams, DrlReplay
    L = _lib()
    vp = ctypes.c_void_p
    d, dc = _desc(294, (128, 64)), _desc(294, (128, 64), 1)
    hp = DQNHParams(batch=1024).c()
    good = DrlReplay(5000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def call(desc=d, h=hp, agent=vp(1 << 20), packed=vp(1 << 21), r=good, size=100):
        return L.drl_dqn_large_train(ctypes.byref(desc), None if h is None else ctypes.byref(h), agent, packed,
                                     None if r is None else ctypes.byref(r), size, None)
    assert call(h=None) != 0 and b"hparams is NULL" in L.drl_last_error()
    assert call(agent=None) != 0 and b"agent block" in L.drl_last_error()
    assert call(agent=vp((1 << 20) + 8)) != 0 and b"16-byte" in L.drl_last_error()
    assert call(packed=None) != 0 and b"packed" in L.drl_last_error()
    assert call(packed=vp((1 << 21) + 4)) != 0 and b"16-byte" in L.drl_last_error()
    assert call(r=None) != 0 and b"replay" in L.drl_last_error()
    assert call(r=DrlReplay(5000, 294, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"NULL" in L.drl_last_error()
    assert call(r=DrlReplay(0, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"capacity" in L.drl_last_error()
    assert call(size=-1) != 0 and b"size" in L.drl_last_error()
    assert call(size=5001) != 0 and b"size" in L.drl_last_error()
    assert call(r=DrlReplay(5000, 292, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0
    assert b"obs_floats" in L.drl_last_error()
    assert call(desc=dc) != 0 and b"policy code" in L.drl_last_error()  # f32 rows for a code net
    assert call(r=DrlReplay(5000, 294, (1 << 20) + 2, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0
    assert b"4-byte" in L.drl_last_error()
    for batch in (0, 4097):
        assert call(h=DQNHParams(batch=batch).c()) != 0 and b"batch" in L.drl_last_error()
    assert call(h=DQNHParams(batch=100, target_update_interval=0).c()) != 0
    assert b"target_update_interval" in L.drl_last_error()
    assert call(h=DQNHParams(batch=100, beta1=1.0).c()) != 0 and b"beta1" in L.drl_last_error()
    bad = _desc(294, (128, 64))
    bad.n_hidden = 4
    assert call(desc=bad) != 0 and b"n_hidden" in L.drl_last_error()
    assert L.drl_dqn_large_init(ctypes.byref(d), 1024, None, 1.0, None) != 0 and b"agent block" in L.drl_last_error()
    assert L.drl_dqn_large_init(ctypes.byref(d), 1024, vp((1 << 20) + 4), 1.0, None) != 0
    assert b"16-byte" in L.drl_last_error()
    assert L.drl_dqn_large_init(ctypes.byref(d), 4097, vp(1 << 20), 1.0, None) != 0 and b"batch" in L.drl_last_error()
    assert L.drl_dqn_large_sample_rows(ctypes.byref(d), ctypes.byref(hp), vp(1 << 20), 100, None, None) != 0
    assert b"d_slots" in L.drl_last_error()
    assert L.drl_dqn_large_sample_rows(ctypes.byref(d), ctypes.byref(hp), vp(1 << 20), 100, vp((1 << 20) + 4), None) != 0
    assert b"d_slots" in L.drl_last_error()
    assert L.drl_dqn_large_sample_rows(ctypes.byref(d), ctypes.byref(hp), None, 100, vp(1 << 20), None) != 0
    assert b"agent block" in L.drl_last_error()
    assert L.drl_dqn_large_sample_rows(ctypes.byref(d), ctypes.byref(hp), vp(1 << 20), 0, vp(1 << 20), None) != 0
    assert b"size" in L.drl_last_error()
    assert L.drl_dqn_large_sample_rows(ctypes.byref(d), None, vp(1 << 20), 10, vp(1 << 20), None) != 0
    assert b"hparams" in L.drl_last_error()


def test_make_learner_dispatch_and_batch_size_option(monkeypatch):
    """make_learner: DQNLearner up to batch 64, LargeBatchDQNLearner above it
    (the classes stubbed: no device); --batch_size 1024 parses into the
    hyperparameters; the limits the two learners name."""
    from dronerl_amd import dqn
    from dronerl_amd.train import hparams_of, parse_args
    made = []
    for name in ("DQNLearner", "LargeBatchDQNLearner"):
        monkeypatch.setattr(dqn, name, lambda net, hp, _n=name, **kw: made.append((_n, hp.batch, kw)) or _n)
    for batch, want in ((1, "DQNLearner"), (8, "DQNLearner"), (64, "DQNLearner"), (65, "LargeBatchDQNLearner"),
                        (1024, "LargeBatchDQNLearner"), (4096, "LargeBatchDQNLearner")):
        assert dqn.make_learner(object(), dqn.DQNHParams(batch=batch), generator=None) == want
        assert made[-1] == (want, batch, {"generator": None})
    assert dqn.make_learner(object()) == "DQNLearner" and made[-1][1] == 8  # (train_jax.py's default batch)
    assert (dqn.DQN_MAX_BATCH, dqn.DQN_LARGE_MAX_BATCH) == (64, 4096)
    a = parse_args(["--batch_size", "1024"])
    assert a.batch_size == 1024 and a.network_type == "dense"
    assert hparams_of(a).batch == 1024
    assert parse_args([]).batch_size == 8


def test_largelearn_layout_places_every_scratch_word_once(tmp_path):
    """tests/native/largelearn_layout_check.cpp, a stand-alone program under
    the address and undefined-behaviour sanitizers: for every (row, layer,
    element) each scratch word is in bounds and distinct, the 16-byte reads
    stay inside their regions and the grids cover every parameter once, at
    batches 1, 65 and 4096 and for the widest net (512-128-128-128-8).
    Nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "largelearn_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "largelearn_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_learn_args_checks_and_fill_on_host_structs(tmp_path):
    """tests/native/learn_args_check.cpp, a stand-alone program under the
    address and undefined-behaviour sanitizers: what every chain learner's
    train call shares behind its plan (csrc/dronerl_learn_args.h and
    per/dronerl_per_learn_args.h), for a dense net at batches 1 and 4096, the
    wide family's 256-wide limit and conv nets at both conv plans, uniform
    and prioritized: each fault of one list is refused with its text, a
    refused call writes nothing, and a good call puts every pointer at the
    fake base + the public layout's offset.  Nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "learn_args_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "learn_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


# Every __global__ kernel under csrc/largelearn/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_dqn_large_rows_kernel": "test_large_batch_learner.py::test_large_learner_matches_oracle_bit_exact",
    "drl_dqn_large_forward_kernel": "test_large_batch_learner.py::test_large_learner_matches_oracle_bit_exact",
    "drl_dqn_large_td_kernel": "test_large_batch_learner.py::test_large_learner_on_a_synthetic_ring_with_invalid_actions",
    "drl_dqn_large_backward_kernel": "test_large_batch_learner.py::test_large_learner_matches_oracle_bit_exact",
    "drl_dqn_large_update_kernel": "test_large_batch_learner.py::test_large_learner_matches_oracle_bit_exact",
    # (the oracle cases start with a ring smaller than the batch: the target blend alone, when due)
    "drl_dqn_large_blend_kernel": "test_large_batch_learner.py::test_large_learner_matches_oracle_bit_exact",
    "drl_dqn_large_counters_kernel": "test_large_batch_learner.py::test_large_learner_matches_oracle_bit_exact",
    "drl_dqn_large_sample_kernel": "test_large_batch_learner.py::test_large_sample_slots_are_the_learners_draws",
}


def test_every_largelearn_kernel_has_a_gpu_test():
    import glob
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "largelearn", "*.hip")):
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
        m = re.search(rf"^@gpu\n(?:@pytest[^\n]*\n)*def {test}\(", text, re.M)
        assert m, (kern, ref)


# ------------------------------------------------------------------- GPU ---
def _host(t):
    return t.detach().cpu().numpy().copy()


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


def _setup(sizes, inp, hp_kw, E, cap, seed=0, cls=None):
    """An env whose window gives sizes[0] inputs, a net with random biases, a
    learner (LargeBatchDQNLearner unless `cls`) with its own target, a ring."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner, ReplayBuffer
    radius = {150: 2, 294: 3}[sizes[0]]
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=radius), E)
    env.reset(seed=seed)
    net, target = _net_and_target(sizes, inp, seed)
    hp = DQNHParams(**hp_kw)
    learner = (cls or LargeBatchDQNLearner)(net, hp, target=target)
    rb = ReplayBuffer(cap, sizes[0], torch.device("cuda"), code_radius=radius if inp == "code" else 0)
    return env, net, learner, rb, hp


class _Loop:
    """train_jax.py's loop shape around a learner: act with the device
    epsilon, step, add_many (the caller trains)."""

    def __init__(self, env, net, learner, rb, inp):
        self.env, self.net, self.learner, self.rb, self.inp = env, net, learner, rb, inp
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
        self.rb.add_many(self.cur, self.acts, r, self.nxt, d)
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


def _oracle_step(st, ohp, rb, code_window):
    return O.learner_step(st, ohp, _host(rb.obs), _host(rb.next_obs), _host(rb.actions), _host(rb.rewards),
                          _host(rb.dones), rb.size, code_window)


def _assert_same(learner, st, where):
    for k in SETS:
        for l, ((w, b), (ow, ob)) in enumerate(zip(learner.params(k), getattr(st, k))):
            assert np.array_equal(_host(w).view(np.uint32), ow.view(np.uint32)), (where, k, l, "W")
            assert np.array_equal(_host(b).view(np.uint32), ob.view(np.uint32)), (where, k, l, "b")
    c = learner.counters()
    assert c["step"] == st.step and c["count"] == st.count, where
    assert np.float32(c["epsilon"]) == st.epsilon and np.float32(c["loss"]) == st.loss, where
    assert c["beta1_pow"] == st.beta1_pow and c["beta2_pow"] == st.beta2_pow, where


def _assert_packed_is_fresh(net):
    """The act's packed image is the online net's: a fresh drl_qnet_pack of
    the same parameters is byte-identical."""
    after = net.packed.clone()
    net.pack()
    torch.cuda.synchronize()
    assert torch.equal(after, net.packed)


# net, input, hyperparameters, envs per step, ring capacity, steps, trained steps at least
ORACLE_CASES = [
    ((294, 128, 64, 5), "code", dict(batch=65), 64, 300, 12, 11),
    # (the ring holds exactly one batch, and wraps)
    ((294, 128, 64, 5), "obs", dict(batch=257, tau=0.6, target_update_interval=3), 50, 257, 12, 7),
    ((294, 96, 32, 32, 5), "code", dict(batch=96, gamma=0.95, learning_rate=3e-3), 40, 500, 12, 10),
    ((150, 64, 5), "obs", dict(batch=130, epsilon_decay_every=1), 64, 200, 12, 10),
    ((294, 16, 16, 5), "code", dict(batch=1000, sample_seed=99), 512, 4000, 8, 7),
    ((294, 128, 64, 5), "code", dict(batch=4096), 2048, 10000, 3, 2),
]
ORACLE_IDS = ["b65", "b257-obs-ring-of-one-batch", "b96-three-hidden", "b130-radius2-obs", "b1000-narrow", "b4096"]


@gpu
@pytest.mark.parametrize("sizes,inp,hp_kw,E,cap,steps,min_trained", ORACLE_CASES, ids=ORACLE_IDS)
def test_large_learner_matches_oracle_bit_exact(sizes, inp, hp_kw, E, cap, steps, min_trained):
    """The train_jax.py loop shape with the large-batch learner on: act
    (device epsilon) -> step -> add_many -> drl_dqn_large_train.  Before each
    train the ring is copied to the host and the oracle takes the same step:
    all four parameter sets, the loss, every counter and both beta powers are
    equal bit for bit after every step, the first ones included, where a ring
    smaller than the batch skips train_step (buffers.py can_sample).  The
    trained-step count follows from E, batch and cap, so no case passes by
    never sampling."""
    env, net, learner, rb, hp = _setup(sizes, inp, hp_kw, E, cap)
    st, ohp = _state(learner), _ohp(hp)
    W = 2 * env.params.window_radius + 1
    loop = _Loop(env, net, learner, rb, inp)
    trained = 0
    for t in range(steps):
        assert np.float32(learner.epsilon.item()) == st.epsilon
        loop.fill()
        trained += _oracle_step(st, ohp, rb, W if inp == "code" else 0)["trained"]
        learner.train(rb)
        torch.cuda.synchronize()
        _assert_same(learner, st, t)
    net.check_errors()
    env.check_errors()
    learner.check_errors()
    assert trained >= min_trained and learner.counters()["count"] == trained
    _assert_packed_is_fresh(net)


@gpu
def test_large_learner_on_a_synthetic_ring_with_invalid_actions():
    """A ring filled from torch with dense randn rows (no zero input, so every
    product counts), a net of 3 actions and actions drawn from {-1, 0, 1, 2,
    7}: a row whose action is outside [0, 3) contributes d = 0 and no delta
    (drl_dqn_train's branch).  Batch 200, 6 steps, bit for bit against the
    oracle; widths 72 and 40 are no multiple of the 16-unit tile."""
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner, ReplayBuffer
    sizes, cap = (150, 72, 40, 3), 700
    net, target = _net_and_target(sizes, "obs", seed=3, n_actions=3)
    hp = DQNHParams(batch=200, tau=0.8, target_update_interval=2, sample_seed=5)
    learner = LargeBatchDQNLearner(net, hp, target=target)
    rb = ReplayBuffer(cap, sizes[0], torch.device("cuda"))
    g = torch.Generator().manual_seed(11)
    rb.obs.copy_(torch.randn((cap, sizes[0]), generator=g))
    rb.next_obs.copy_(torch.randn((cap, sizes[0]), generator=g))
    choice = torch.tensor([-1, 0, 1, 2, 7], dtype=torch.int32)
    rb.actions.copy_(choice[torch.randint(0, 5, (cap,), generator=g)])
    rb.rewards.copy_(torch.randn(cap, generator=g))
    rb.dones.copy_((torch.rand(cap, generator=g) < 0.2).to(torch.uint8))
    rb.size, rb.cursor = cap, 0
    st, ohp = _state(learner), _ohp(hp)
    acts_host, invalid = _host(rb.actions), 0
    for t in range(6):
        info = _oracle_step(st, ohp, rb, 0)
        invalid += sum(1 for s in info["rows"] if not 0 <= int(acts_host[s]) < 3)
        learner.train(rb)
        torch.cuda.synchronize()
        _assert_same(learner, st, t)
    assert invalid > 100 and learner.counters()["count"] == 6
    learner.check_errors()
    _assert_packed_is_fresh(net)


@gpu
@pytest.mark.parametrize("batch", [8, 64])
def test_large_learner_equals_the_single_launch_learner(batch):
    """At batches drl_dqn_train takes, the launch chain leaves the same state:
    both learners from identical initial states on the same ring for 12 steps
    (the ring starts smaller than batch 64): the blocks' parameter sets, the
    counters and the packed images are equal bit for bit."""
    from dronerl_amd.dqn import DQNLearner, LargeBatchDQNLearner
    sizes, kw = (294, 128, 64, 5), dict(batch=batch, tau=0.7, target_update_interval=3)
    env, net_a, a, rb, _ = _setup(sizes, "code", kw, 40, 300, cls=DQNLearner)
    _, net_b, b, _, _ = _setup(sizes, "code", kw, 40, 300, cls=LargeBatchDQNLearner)
    assert isinstance(b, LargeBatchDQNLearner) and not isinstance(a, LargeBatchDQNLearner)
    for k in SETS:
        assert torch.equal(a.sets[k].view(torch.int32), b.sets[k].view(torch.int32)), k
    loop = _Loop(env, net_a, a, rb, "code")
    for t in range(12):
        loop.fill()
        a.train(rb)
        b.train(rb)
        torch.cuda.synchronize()
        for k in SETS:
            assert torch.equal(a.sets[k].view(torch.int32), b.sets[k].view(torch.int32)), (t, k)
        assert a.counters() == b.counters(), t
        assert torch.equal(net_a.packed, net_b.packed), t
    assert a.counters()["count"] == (12 if batch == 8 else 11)
    a.check_errors()
    b.check_errors()


@functools.lru_cache(maxsize=None)
def _code_ring(cap):
    """A full ring of policy-code transitions (shared, read only)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import ReplayBuffer
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), cap)
    env.reset(seed=7)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    acts = env.synth_actions(seed=9, step=0)
    r, d = env.step(acts, code=nxt)
    rb.add_many(cur, acts, r, nxt, d)
    torch.cuda.synchronize()
    assert rb.size == cap
    return rb


@gpu
def test_large_sample_slots_are_the_learners_draws():
    """LargeBatchDQNLearner.sample_slots (drl_dqn_large_sample_rows) == the
    oracle's sample_indices at the device step, step after step, for a batch
    of 300 (more than one workgroup of the sample kernel); refused for an
    empty ring."""
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner
    from dronerl_amd.handle import DroneRLError
    rb = _code_ring(900)
    net, target = _net_and_target((294, 16, 16, 5), "code", seed=2)
    learner = LargeBatchDQNLearner(net, DQNHParams(batch=300, sample_seed=77), target=target)
    for t in range(4):
        for size in (300, 555, 900):
            assert learner.sample_slots(size).cpu().tolist() == O.sample_indices(77, t, 300, size), (t, size)
        learner.train(rb)
    torch.cuda.synchronize()
    assert learner.counters()["step"] == 4 and learner.counters()["count"] == 4
    with pytest.raises(DroneRLError):
        learner.sample_slots(0)
    with pytest.raises(ValueError):
        learner.sample_slots(900, out=torch.empty(299, dtype=torch.int64, device="cuda"))


@gpu
def test_large_learner_is_graph_capturable():
    """One train() (batch 257) captured with torch.cuda.graph and replayed 6
    times equals 6 eager calls on a twin learner bit for bit: a replay
    continues the schedule, because the step, Adam's count and epsilon live on
    the device and the row draw reads the device step."""
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner
    rb = _code_ring(900)
    hp = DQNHParams(batch=257, tau=0.6, target_update_interval=3, epsilon_decay_every=2)

    def make():
        net, target = _net_and_target((294, 128, 64, 5), "code", seed=4)
        return net, LargeBatchDQNLearner(net, hp, target=target)

    (net_e, eager), (net_g, graphed) = make(), make()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed.train(rb)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert graphed.counters()["step"] == 0  # (capturing runs nothing)
    for _ in range(6):
        g.replay()
        eager.train(rb)
    torch.cuda.synchronize()
    assert eager.counters()["step"] == 6 and eager.counters()["count"] == 6
    for k in SETS:
        assert torch.equal(eager.sets[k].view(torch.int32), graphed.sets[k].view(torch.int32)), k
    assert eager.counters() == graphed.counters()
    assert torch.equal(net_e.packed, net_g.packed)
    _assert_packed_is_fresh(net_g)


# ---- two gloo ranks sharing the GPU (as tests/test_gpu_multirank.py's global learner) ----
GL_STEPS, GL_BATCH, GL_E, GL_CAP = 12, 96, 256, 1000


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gl_run(rank, world):
    """train_jax.py's loop over one shard (world > 1: ShardedReplay + gather
    before every learner step) or over every env (world == 1: the plain ring)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.distributed import shard_envs
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner, QNetwork, ReplayBuffer, make_learner
    from dronerl_amd.global_learner import ShardedReplay
    sh = shard_envs(GL_E, rank, world)
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), sh.num_envs, device="cuda:0",
                                env_offset=sh.env_offset)
    env.reset(seed=21)
    net = QNetwork(294, (128, 64), device="cuda:0", generator=torch.Generator().manual_seed(3), input="code")
    learner = make_learner(net, DQNHParams(batch=GL_BATCH, target_update_interval=3),
                           generator=torch.Generator().manual_seed(4))
    assert isinstance(learner, LargeBatchDQNLearner)
    if world > 1:
        sr = ShardedReplay(GL_CAP, 294, torch.device("cuda:0"), GL_E, sh.env_offset, sh.num_envs, rank, world,
                           code_radius=3)
        ring = sr.ring
    else:
        sr = ring = ReplayBuffer(GL_CAP, 294, torch.device("cuda:0"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    acts = torch.empty((sh.num_envs, 8), dtype=torch.int32, device="cuda:0")
    for t in range(GL_STEPS):
        net.act(cur, learner.epsilon, seed=9, step=t, env_offset=sh.env_offset, actions=acts, synth=(13, t))
        r, d = env.step(acts, code=nxt)
        sr.add_many(cur, acts, r, nxt, d)
        if world > 1:
            sr.gather(learner)
        learner.train(ring)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    learner.check_errors()
    out = {k: learner.sets[k].cpu().numpy().copy() for k in SETS}
    out["counters"] = learner.counters()
    out["packed"] = net.packed.cpu().numpy().copy()
    return out


def _gl_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out[rank] = _gl_run(rank, world)
    finally:
        dist.destroy_process_group()


@gpu
def test_large_learner_two_ranks_equal_one_learner():
    """Two ranks, each with half the envs, its own image of the global ring and
    the exchange of the 96 drawn rows before every learner step
    (ShardedReplay.gather needs only hp.batch and sample_slots), end with
    parameters, target, Adam moments, counters and packed image all equal, bit
    for bit, to one learner over every env's transitions in one ring."""
    ref = _gl_run(0, 1)
    assert ref["counters"]["count"] == GL_STEPS
    ctx = mp.get_context("spawn")
    with ctx.Manager() as man:
        out = man.dict()
        port = _free_port()
        procs = [ctx.Process(target=_gl_worker, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
            assert p.exitcode == 0, p.exitcode
        res = dict(out)
    for r in range(2):
        for k in (*SETS, "packed"):
            assert np.array_equal(res[r][k].view(np.uint32), ref[k].view(np.uint32)), (r, k)
        assert res[r]["counters"] == ref["counters"], r


@gpu
def test_train_main_cli_with_a_large_batch(tmp_path):
    """`python -m dronerl_amd.train --batch_size 128` just works: train with
    the large-batch learner, run the final eval, return the metrics."""
    from dronerl_amd.train import main
    m = main(["--num_envs", "512", "--num_steps", "60", "--batch_size", "128", "--num_evals", "3",
              "--num_eval_steps", "200", "--output_dir", str(tmp_path)])
    assert m["obs_per_sec"] > 0 and m["num_gpus"] == 1
    assert -1.0 <= m["eval_reward_mean"] <= 1.0 and -1.0 <= m["random_reward_mean"] <= 1.0


# The measured greedy-eval gaps (drone 0's mean reward minus the random drones') after 300 steps of 4096 envs, in
# one run (profiles/large_batch/train_eval.json): batch 256: 0.1276 (agent -0.0475, random -0.1752); batch 8
# (drl_dqn_train): 0.0817 (agent -0.1017, random -0.1834).  The batch-256 run repeated in the same process gave
# the same figures to the last bit.  The test asserts half the batch-256 gap.
MEASURED_GAP_256 = 0.1276


@gpu
def test_agent_trained_with_a_large_batch_beats_random():
    """train(EnvParams(), 4096, 300) with batch 256, then the greedy eval_jax
    of the learned parameters as tests/test_train.py runs it: drone 0's reward
    is above the random drones' by at least half the measured gap (the run is
    deterministic: every kernel is bit-reproducible)."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner, QNetwork
    from dronerl_amd.train import evaluate, train
    p = EnvParams()
    res = train(p, 4096, 300, hp=DQNHParams(batch=256, num_steps=300))
    assert isinstance(res.learner, LargeBatchDQNLearner)
    c = res.learner.counters()
    assert c["step"] == 300 and c["count"] == 300
    qnet = QNetwork(294, (128, 64), precision="f32")
    qnet.load(*zip(*res.learner.params("online")))
    agent, rnd, table = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
    print(f"eval after 300 steps at batch 256: agent {agent[0]:.4f} +- {agent[1]:.4f}, "
          f"random {rnd[0]:.4f} +- {rnd[1]:.4f}, gap {agent[0] - rnd[0]:.4f}")
    assert table.shape == (5, 2)
    assert agent[0] > rnd[0] + MEASURED_GAP_256 / 2, (agent, rnd)
