"""The DQN learner for conv Q-networks: drl_convnet_dqn_* (dronerl_amd/csrc/convlearn/),
dronerl_amd.dqn.ConvDQNLearner, checkpoint.save_conv and
`python -m dronerl_amd.train --network_type conv`.

Reference: train_jax.py:68-98 with network_type == 'conv' (jax dqn.py:66-94,
147-200), optax.adam.  The checker is tests/_conv_learner_ref.py: a torch
restatement (autograd + the Adam formula written out) in f64 and in f32.  The
device is compared with the f64 one per step, after the reference is loaded
with the device's own state; the tolerance is derived from the f32
restatement alone (_conv_learner_ref.tolerance) and may never exceed 1e-4.
"""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _conv_learner_ref as R
from oracle import dqn_learner as O

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(REPO, "tests", "golden")
TOL_CAP = 1e-4
STEPS = 30
SETS = ("online", "target", "m", "v")


def _ohp(batch, kw):
    """oracle HParams of a case: train_jax.py's defaults for a 1000-step run, then the case's own."""
    base = dict(batch=batch, epsilon_decay=O.train_jax_epsilon_decay(1000))
    base.update(kw)
    return O.HParams(**base)


# ------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
@pytest.mark.parametrize("bias_std", [0.0, 0.05])
def test_tolerance_condition_holds_on_the_references_alone(case, bias_std):
    """The tolerance the GPU test computes (max(1e-5, 4 x the f32 restatement's
    distance from the f64 one)) stays within 1e-4: checked with the two
    references alone on synthetic windows, every case's net, batch and
    hyperparameters, zero and random biases, from zero moments on."""
    name, _, batch, kw, cap = case
    W, conv, dense = R.NETS[name]
    hp = _ohp(batch, kw)
    seed = sum(map(ord, name))
    g = np.random.default_rng(seed)
    obs, nxt = R.synthetic_windows(W, cap, seed + 1), R.synthetic_windows(W, cap, seed + 2)
    act = g.integers(0, 5, cap).astype(np.int32)
    rew = g.choice(np.array([0.0, 1.0, -1.0, -0.1], np.float32), cap)
    done = (g.random(cap) < 0.1).astype(np.uint8)
    st = {"online": R.random_params(W, conv, dense, seed + 3, bias_std),
          "target": R.random_params(W, conv, dense, seed + 4, bias_std), "step": 0, "count": 0}
    st["m"] = [(np.zeros_like(w), np.zeros_like(b)) for w, b in st["online"]]
    st["v"] = [(np.zeros_like(w), np.zeros_like(b)) for w, b in st["online"]]
    worst = 0.0
    for step in range(8):
        idx = O.sample_indices(hp.sample_seed, step, batch, cap)
        r64 = R.ref_step(st, hp, W, conv, obs[idx], nxt[idx], act[idx], rew[idx], done[idx], torch.float64)
        r32 = R.ref_step(st, hp, W, conv, obs[idx], nxt[idx], act[idx], rew[idx], done[idx], torch.float32)
        for k in SETS:
            for (a, b), (e, f) in zip(r32[k], r64[k]):
                worst = max(worst, R.tolerance(a, e), R.tolerance(b, f))
        worst = max(worst, R.tolerance(r32["loss"], r64["loss"]))
        for k in SETS:  # the next step starts from f32 state, as the device's does
            st[k] = [(w.astype(np.float32), b.astype(np.float32)) for w, b in r64[k]]
        st["step"] += 1
        st["count"] += 1
    print(f"{name}: worst tolerance {worst:.3g}")
    assert worst <= TOL_CAP


def _desc(name, inp="obs", n_actions=5):
    from dronerl_amd.dqn import convnet_desc
    W, conv, dense = R.NETS[name]
    return convnet_desc((W, W, 6), conv, dense, n_actions, inp)


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind, _bind_convnet
    return _bind(_bind_convnet(lib()))


def test_convnet_dqn_layout_query():
    """Host only: offsets disjoint and aligned, n_params the sum of the
    layers, the refusals by name."""
    from dronerl_amd.dqn import DrlConvnetDqnLayout
    L = _lib()
    for name, (W, conv, dense) in R.NETS.items():
        for batch in (1, 8, 64):
            lay = DrlConvnetDqnLayout()
            assert L.drl_convnet_dqn_layout_query(ctypes.byref(_desc(name)), batch, ctypes.byref(lay)) == 0, \
                L.drl_last_error()
            shp = R.shapes(W, conv, dense)
            assert lay.n_layers == len(shp)
            off = 0
            for l, (ws, bs) in enumerate(shp):
                assert lay.weight_off[l] == off
                off += int(np.prod(ws))
                assert lay.bias_off[l] == off
                off += bs[0]
            assert lay.n_params == off
            marks = [lay.online_off, lay.target_off, lay.m_off, lay.v_off, lay.counters_off, lay.scratch_off,
                     lay.bytes]
            need = [4 * off] * 4 + [64, batch * lay.row_bytes]
            assert marks[0] == 0 and all(m % 16 == 0 for m in marks[:-1])
            assert all(marks[i] + need[i] <= marks[i + 1] for i in range(6))
            assert 0 < lay.row_bytes <= 65536
    lay = DrlConvnetDqnLayout()
    d = _desc("a")
    for batch in (0, 65):
        assert L.drl_convnet_dqn_layout_query(ctypes.byref(d), batch, ctypes.byref(lay)) != 0
        assert b"batch" in L.drl_last_error()
    assert L.drl_convnet_dqn_layout_query(None, 8, ctypes.byref(lay)) != 0 and b"NULL" in L.drl_last_error()
    assert L.drl_convnet_dqn_layout_query(ctypes.byref(d), 8, None) != 0 and b"layout is NULL" in L.drl_last_error()
    bad = _desc("a")
    bad.conv[0].kernel_size = 6
    assert L.drl_convnet_dqn_layout_query(ctypes.byref(bad), 8, ctypes.byref(lay)) != 0
    assert b"kernel_size" in L.drl_last_error()
    from dronerl_amd.dqn import convnet_desc
    wide = convnet_desc((9, 9, 6), ({"out_channels": 32, "kernel_size": 1, "stride": 1, "padding": 4},))
    assert L.drl_convnet_dqn_layout_query(ctypes.byref(wide), 8, ctypes.byref(lay)) != 0
    assert b"DRL_CONVNET_DQN_ROW_BYTES_MAX" in L.drl_last_error()


def test_convnet_dqn_calls_validate_before_device_work():
    """Every pointer, the alignment, the batch and the size are checked
    before any device work (no GPU needed)."""
    from dronerl_amd.dqn import DQNHParams, DrlReplay
    L = _lib()
    vp = ctypes.c_void_p
    d, dc = _desc("a"), _desc("a", "code")
    hp = DQNHParams(batch=8).c()
    good = DrlReplay(1000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def call(desc=d, h=hp, agent=vp(1 << 20), packed=vp(1 << 21), r=good, size=100):
        return L.drl_convnet_dqn_train(ctypes.byref(desc), None if h is None else ctypes.byref(h), agent, packed,
                                       None if r is None else ctypes.byref(r), size, None)
    assert call(h=None) != 0 and b"hparams is NULL" in L.drl_last_error()
    assert call(agent=None) != 0 and b"agent block" in L.drl_last_error()
    assert call(agent=vp((1 << 20) + 8)) != 0 and b"16-byte" in L.drl_last_error()
    assert call(packed=None) != 0 and b"packed" in L.drl_last_error()
    assert call(packed=vp((1 << 21) + 4)) != 0 and b"16-byte" in L.drl_last_error()
    assert call(r=None) != 0 and b"replay" in L.drl_last_error()
    assert call(r=DrlReplay(1000, 294, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"NULL" in L.drl_last_error()
    assert call(size=-1) != 0 and b"size" in L.drl_last_error()
    assert call(size=1001) != 0 and b"size" in L.drl_last_error()
    assert call(r=DrlReplay(1000, 292, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0
    assert b"obs_floats" in L.drl_last_error()
    assert call(desc=dc) != 0 and b"policy code" in L.drl_last_error()  # f32 rows for a code net
    assert call(r=DrlReplay(1000, 294, (1 << 20) + 2, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0
    assert b"4-byte" in L.drl_last_error()
    for batch in (0, 65):
        assert call(h=DQNHParams(batch=batch).c()) != 0 and b"batch" in L.drl_last_error()
    assert call(h=DQNHParams(batch=8, target_update_interval=0).c()) != 0 and b"target_update_interval" in L.drl_last_error()
    assert call(h=DQNHParams(batch=8, beta1=1.0).c()) != 0 and b"beta1" in L.drl_last_error()
    assert L.drl_convnet_dqn_init(ctypes.byref(d), 8, None, 1.0, None) != 0 and b"agent block" in L.drl_last_error()
    assert L.drl_convnet_dqn_init(ctypes.byref(d), 65, vp(1 << 20), 1.0, None) != 0 and b"batch" in L.drl_last_error()
    assert L.drl_convnet_dqn_sample_rows(ctypes.byref(d), ctypes.byref(hp), vp(1 << 20), 100, None, None) != 0
    assert b"d_slots" in L.drl_last_error()
    assert L.drl_convnet_dqn_sample_rows(ctypes.byref(d), ctypes.byref(hp), vp(1 << 20), 0, vp(1 << 20), None) != 0
    assert b"size" in L.drl_last_error()
    assert L.drl_convnet_dqn_sample_rows(ctypes.byref(d), None, vp(1 << 20), 10, vp(1 << 20), None) != 0
    assert b"hparams" in L.drl_last_error()


def test_convlearn_layout_maps_every_parameter_and_scratch_word_once(tmp_path):
    """tests/native/convlearn_layout_check.cpp, a stand-alone program under
    the address and undefined-behaviour sanitizers: the parameter index <->
    (layer, co, ci, ky, kx) map is a bijection and every scratch word of every
    (row, layer, element) is in bounds and distinct, for cases a-i and the
    limits' corners.  Nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "convlearn_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "convlearn_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_save_conv_torch_agent_reproduces_the_reference_file(tmp_path):
    """save_conv(format="torch_agent") of dqn-agent-5's own tensors == that
    file (the reference's torch DQNAgent.save wrote it): metadata and tensors."""
    from dronerl_amd.checkpoint import read_checkpoint, save_conv
    src = os.path.join(GOLD, "sample_models", "dqn-agent-5.safetensors")
    ck = read_checkpoint(src)
    t = ck.tensors
    out = str(tmp_path / "agent5.safetensors")
    save_conv(out, [t["network.conv2d_1.weight"]], [t["network.conv2d_1.bias"]],
              [t["network.dense_1.weight"], t["network.dense_2.weight"]],
              [t["network.dense_1.bias"], t["network.dense_2.bias"]], ck.obs_shape, ck.conv_layers,
              format="torch_agent")
    back = read_checkpoint(out)
    assert back.metadata == ck.metadata
    assert sorted(back.tensors) == sorted(t)
    for k in t:
        assert back.tensors[k].dtype == t[k].dtype and np.array_equal(back.tensors[k], t[k]), k


def test_save_conv_jax_and_torch_round_trip_with_the_transposes(tmp_path):
    """The "jax" and "torch" forms through read_checkpoint: names (Conv_i <->
    conv2d_{i+1}), the (2, 3, 1, 0) / (3, 2, 0, 1) kernel transposes on a
    kernel whose every element differs, and the metadata rules."""
    from safetensors import safe_open
    from dronerl_amd.checkpoint import read_checkpoint, save_conv
    W, conv, dense = R.NETS["c"]
    shp = R.shapes(W, conv, dense)
    ps = [(np.arange(int(np.prod(ws)), dtype=np.float32).reshape(ws) + 1000 * l,
           np.arange(bs[0], dtype=np.float32) - l) for l, (ws, bs) in enumerate(shp)]
    cw, cb = [p[0] for p in ps[:2]], [p[1] for p in ps[:2]]
    dw, db = [p[0] for p in ps[2:]], [p[1] for p in ps[2:]]
    given = ({"kernel_size": 3, "out_channels": 8}, {"kernel_size": 3, "out_channels": 12, "stride": 2, "padding": 1})
    for fmt in ("jax", "torch"):
        path = str(tmp_path / f"c_{fmt}.safetensors")
        save_conv(path, cw, cb, dw, db, (W, W, 6), given, format=fmt, hidden_layers=(16, 16))
        with safe_open(path, framework="numpy") as f:
            md, raw = f.metadata(), {k: f.get_tensor(k) for k in f.keys()}
        assert md["network_type"] == "conv" and md["checkpoint_format"] == fmt
        assert md["conv_layers"] == str(given) and md["conv_dense_layers"] == "(16, 8)"
        assert md["dense_layers"] == ("(16, 16)" if fmt == "jax" else "(16, 8)")  # jax dqn.py:293 / :314-315
        assert md["obs_shape"] == "(9, 9, 6)" and md["action_shape"] == "(5,)"
        if fmt == "jax":
            assert raw["params.Conv_1.kernel"].shape == (3, 3, 8, 12)
            assert raw["params.Conv_1.kernel"][1, 2, 5, 7] == cw[1][7, 5, 1, 2]
            assert raw["params.Dense_0.kernel"].shape == dw[0].shape[::-1]
            assert raw["params.Dense_0.kernel"][3, 4] == dw[0][4, 3]
        else:
            assert np.array_equal(raw["network.conv2d_2.weight"], cw[1])
        ck = read_checkpoint(path)
        assert ck.network_type == "conv" and ck.dense_layers == (16, 8) and tuple(ck.obs_shape) == (9, 9, 6)
        assert [dict(c) for c in ck.conv_layers] == [dict(c) for c in given]
        for i in range(2):
            assert np.array_equal(ck.tensors[f"network.conv2d_{i + 1}.weight"], cw[i])
            assert np.array_equal(ck.tensors[f"network.conv2d_{i + 1}.bias"], cb[i])
        for i in range(3):
            assert np.array_equal(ck.tensors[f"network.dense_{i + 1}.weight"], dw[i])
            assert np.array_equal(ck.tensors[f"network.dense_{i + 1}.bias"], db[i])
    with pytest.raises(ValueError):
        save_conv(str(tmp_path / "x"), cw, cb, dw[1:], db[1:], (W, W, 6), given)  # 16 columns on a flatten of 192


def test_parse_args_conv_options_and_sharding_refusal():
    from dronerl_amd.train import parse_args
    a = parse_args([])
    assert a.network_type == "dense" and tuple(a.hidden_layers) == (128, 64) and tuple(a.conv_dense_layers) == ()
    assert a.conv_layers == ({"kernel_size": 3, "out_channels": 8, "padding": 1, "stride": 1},)  # train_jax.py:366
    a = parse_args(["--network_type", "conv", "--conv_dense_layers", "16", "8", "--conv_layers",
                    '[{"out_channels": 4, "kernel_size": 3, "padding": 1}, {"out_channels": 6, "kernel_size": 2}]'])
    assert a.network_type == "conv" and list(a.conv_dense_layers) == [16, 8]
    assert a.conv_layers == ({"out_channels": 4, "kernel_size": 3, "padding": 1}, {"out_channels": 6, "kernel_size": 2})
    assert parse_args(["--conv_layers", "{'out_channels': 4, 'kernel_size': 3}"]).conv_layers == \
        ({"out_channels": 4, "kernel_size": 3},)
    with pytest.raises(SystemExit):
        parse_args(["--network_type", "lstm"])
    with pytest.raises(SystemExit):
        parse_args(["--conv_layers", "[{"])
    with pytest.raises(ValueError, match="use_sharding with --network_type conv"):
        parse_args(["--network_type", "conv", "--use_sharding", "--num_envs", "8"])
    parse_args(["--network_type", "dense", "--use_sharding", "--num_envs", "8"])


# Every __global__ kernel under csrc/convlearn/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_convnet_dqn_rows_kernel": "test_convnet_learner.py::test_learner_matches_the_restatement_per_step",
    "drl_convnet_dqn_update_kernel": "test_convnet_learner.py::test_learner_matches_the_restatement_per_step",
    "drl_convnet_dqn_counters_kernel": "test_convnet_learner.py::test_learner_without_a_sample_only_schedules",
}


def test_every_convlearn_kernel_has_a_gpu_test():
    import glob
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "convlearn", "*.hip")):
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


@functools.lru_cache(maxsize=None)
def _ring(W, inp, cap):
    """A replay ring of `cap` slots filled from 64 envs x 5 steps (16 x 16, 8 drones) with real windows of side
    W: f32 rows or policy-code rows.  Shared by the tests (read only)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import ReplayBuffer
    r, E = (W - 1) // 2, 64
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=r), E)
    env.reset(seed=0)
    rb = ReplayBuffer(cap, W * W * 6, torch.device("cuda"), code_radius=r if inp == "code" else 0)
    code = inp == "code"
    cur = env.new_code() if code else torch.empty((E, 1, W, W, 6), device="cuda")
    nxt = env.new_code() if code else torch.empty((E, 1, W, W, 6), device="cuda")
    if code:
        env.get_code(out=cur)
    else:
        env.get_obs(1, out=cur)
    for t in range(5):
        acts = env.synth_actions(seed=9, step=t)
        if code:
            rew, don = env.step(acts, code=nxt)
        else:
            rew, don, _ = env.step(acts, obs_k=1, obs=nxt)
        rb.add_many(cur, acts, rew, nxt, don)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    env.check_errors()
    assert rb.size == min(cap, 320)
    host = {"obs": _host(rb.obs), "next_obs": _host(rb.next_obs), "actions": _host(rb.actions),
            "rewards": _host(rb.rewards), "dones": _host(rb.dones)}
    return rb, host


def _rows(host, idx, W, inp):
    if inp == "code":
        return O.decode_code_rows(host["obs"][idx], W), O.decode_code_rows(host["next_obs"][idx], W)
    return host["obs"][idx, :W * W * 6], host["next_obs"][idx, :W * W * 6]


def _learner(name, inp, batch, kw, seed=0, bias_std=0.05):
    from dronerl_amd.dqn import ConvDQNLearner, ConvQNetwork, DQNHParams
    W, conv, dense = R.NETS[name]
    net = ConvQNetwork((W, W, 6), conv, dense, generator=torch.Generator().manual_seed(seed + 5), input=inp)
    if bias_std:
        on = R.random_params(W, conv, dense, seed + 6, bias_std)
        nc = len(conv)
        net.load(net.conv_weights, [torch.tensor(b) for _, b in on[:nc]], net.weights,
                 [torch.tensor(b) for _, b in on[nc:]])
    tg = R.random_params(W, conv, dense, seed + 7, bias_std)
    nc = len(conv)
    target = ([torch.tensor(w) for w, _ in tg[:nc]], [torch.tensor(b) for _, b in tg[:nc]],
              [torch.tensor(w) for w, _ in tg[nc:]], [torch.tensor(b) for _, b in tg[nc:]])
    hp = DQNHParams(batch=batch, num_steps=1000, **kw)
    return net, ConvDQNLearner(net, hp, target=target), hp


def _state(learner):
    st = {k: [(_host(w), _host(b)) for w, b in learner.params(k)] for k in SETS}
    st.update(learner.counters())
    return st


@gpu
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_learner_matches_the_restatement_per_step(case):
    """30 learner steps on a filled ring.  Before each step the f64 and f32
    restatements are loaded with the device's own state (the four sets, the
    counters) and the rows of oracle.sample_indices; after it, online, target,
    mu and nu of every layer and the loss are within the derived tolerance of
    the f64 one; step, count, epsilon and the beta powers are exact, and on a
    tau = 1 update step the target is the new online set bit for bit."""
    name, inp, batch, kw, cap = case
    W, conv, dense = R.NETS[name]
    rb, host = _ring(W, inp, cap)
    net, learner, hp = _learner(name, inp, batch, kw, bias_std=0.0 if name == "b" else 0.05)
    ohp = O.HParams(batch=hp.batch, gamma=hp.gamma, learning_rate=hp.learning_rate, beta1=hp.beta1, beta2=hp.beta2,
                    adam_eps=hp.adam_eps, tau=hp.tau, target_update_interval=hp.target_update_interval,
                    epsilon_decay=hp.decay(), epsilon_end=hp.epsilon_end,
                    epsilon_decay_every=hp.epsilon_decay_every, sample_seed=hp.sample_seed)
    worst_tol = worst = 0.0
    for step in range(STEPS):
        st = _state(learner)
        assert st["step"] == step and st["count"] == step
        idx = O.sample_indices(hp.sample_seed, step, batch, rb.size)
        X, Xn = _rows(host, idx, W, inp)
        args = (st, ohp, W, conv, X, Xn, host["actions"][idx], host["rewards"][idx], host["dones"][idx])
        r64, r32 = R.ref_step(*args, torch.float64), R.ref_step(*args, torch.float32)
        learner.train(rb)
        dev = _state(learner)
        tol = R.tolerance(r32["loss"], r64["loss"])
        assert tol <= TOL_CAP and R.rel(dev["loss"], r64["loss"]) <= tol, (step, "loss", dev["loss"], r64["loss"])
        for k in SETS:
            for l, ((a, b), (e32, f32), (e, f)) in enumerate(zip(dev[k], r32[k], r64[k])):
                for what, got, lo, hi in (("W", a, e32, e), ("b", b, f32, f)):
                    tol = R.tolerance(lo, hi)
                    dist = R.rel(got, hi)
                    worst_tol, worst = max(worst_tol, tol), max(worst, dist)
                    assert tol <= TOL_CAP and dist <= tol, (step, k, l, what, dist, tol)
        # the schedule, exactly
        assert dev["step"] == step + 1 and dev["count"] == step + 1
        eps = np.float32(st["epsilon"])
        if step % hp.epsilon_decay_every == 0:
            eps = max(np.float32(eps * np.float32(hp.decay())), np.float32(hp.epsilon_end))
        assert np.float32(dev["epsilon"]) == eps, step
        assert dev["beta1_pow"] == st["beta1_pow"] * hp.beta1 and dev["beta2_pow"] == st["beta2_pow"] * hp.beta2
        due = step % hp.target_update_interval == 0
        for (tw, tb), (ow, ob), (pw, pb) in zip(dev["target"], dev["online"], st["target"]):
            if due and hp.tau == 1.0:
                assert np.array_equal(tw.view(np.uint32), ow.view(np.uint32)) and np.array_equal(tb, ob), step
            elif not due:
                assert np.array_equal(tw.view(np.uint32), pw.view(np.uint32)) and np.array_equal(tb, pb), step
    print(f"{name}: worst distance {worst:.3g}, worst tolerance {worst_tol:.3g}")
    learner.check_errors()
    net.check_errors()


@gpu
def test_learner_is_reproducible_and_graph_capturable():
    """Two learners from the same state on the same ring, 10 steps: all four
    sets and the counters are bit-identical.  One train() captured with
    torch.cuda.graph and replayed 5 times equals 5 eager calls bit for bit (a
    replay continues the schedule: the counters live on the device)."""
    rb, _ = _ring(9, "code", 300)
    kw = dict(tau=0.6, target_update_interval=3)

    def same(a, b):
        for k in SETS:
            if not torch.equal(a.sets[k].view(torch.int32), b.sets[k].view(torch.int32)):
                return False
        return torch.equal(a._ctr_i, b._ctr_i) and torch.equal(a.net.packed, b.net.packed)

    _, a, _ = _learner("c", "code", 5, kw)
    _, b, _ = _learner("c", "code", 5, kw)
    assert same(a, b)
    for _ in range(10):
        a.train(rb)
    for _ in range(10):
        b.train(rb)
    torch.cuda.synchronize()
    assert same(a, b) and a.counters()["count"] == 10
    _, eager, _ = _learner("c", "code", 5, kw)
    _, graphed, _ = _learner("c", "code", 5, kw)
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
    for _ in range(5):
        g.replay()
        eager.train(rb)
    torch.cuda.synchronize()
    assert eager.counters()["step"] == 5 and same(eager, graphed)


@gpu
@pytest.mark.parametrize("name,inp", [("a", "obs"), ("c", "code")])
def test_packed_image_follows_the_learned_parameters(name, inp):
    """After each of 5 steps net.packed is byte-equal to the image of a fresh
    ConvQNetwork loaded with the learned parameters, and the act's Q on 17
    windows is equal too."""
    from dronerl_amd.dqn import ConvQNetwork
    W, conv, dense = R.NETS[name]
    rb, _ = _ring(W, inp, 300)
    net, learner, _ = _learner(name, inp, 8, {})
    x = rb.obs[:17].contiguous()
    q_live, q_fresh = torch.empty((17, 5), device="cuda"), torch.empty((17, 5), device="cuda")
    for step in range(5):
        learner.train(rb)
        fresh = ConvQNetwork((W, W, 6), conv, dense, input=inp)
        fresh.load(net.conv_weights, net.conv_biases, net.weights, net.biases)
        torch.cuda.synchronize()
        assert torch.equal(net.packed, fresh.packed), step
        net.act(x, 0.0, q_out=q_live)
        fresh.act(x, 0.0, q_out=q_fresh)
        assert torch.equal(q_live, q_fresh), step
    before = net.packed.clone()
    net.pack()
    assert torch.equal(before, net.packed)
    learner.check_errors()


@gpu
def test_learner_without_a_sample_only_schedules():
    """size < batch (buffers.py can_sample): parameters and moments
    untouched, loss 0, count 0; step advances, epsilon decays, and the target
    blends at step 0 (and not at step 1)."""
    from dronerl_amd.dqn import ReplayBuffer
    rb, _ = _ring(7, "obs", 300)
    small = ReplayBuffer(300, 294, torch.device("cuda"))
    small.obs.copy_(rb.obs)
    small.next_obs.copy_(rb.next_obs)
    small.size = small.cursor = 7
    net, learner, hp = _learner("a", "obs", 8, dict(tau=0.25, epsilon_decay_every=1))
    before = _state(learner)
    learner.train(small)
    after = _state(learner)
    for k in ("online", "m", "v"):
        for (a, b), (c, d) in zip(before[k], after[k]):
            assert np.array_equal(a, c) and np.array_equal(b, d), k
    for (tw, tb), (ow, ob), (pw, pb) in zip(after["target"], before["online"], before["target"]):
        assert np.array_equal(tw, np.float32(0.25) * ow + np.float32(0.75) * pw)
        assert np.array_equal(tb, np.float32(0.25) * ob + np.float32(0.75) * pb)
    assert after["step"] == 1 and after["count"] == 0 and after["loss"] == 0.0
    assert after["beta1_pow"] == 1.0 and after["beta2_pow"] == 1.0
    assert np.float32(after["epsilon"]) == np.float32(np.float32(1.0) * np.float32(hp.decay()))
    learner.train(small)  # step 1: no blend
    again = _state(learner)
    for (a, b), (c, d) in zip(after["target"], again["target"]):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    assert again["step"] == 2 and again["count"] == 0
    fresh_image = net.packed.clone()
    net.pack()
    assert torch.equal(fresh_image, net.packed)


@gpu
def test_sample_slots_are_the_learners_draws():
    """ConvDQNLearner.sample_slots (drl_convnet_dqn_sample_rows) == oracle.
    sample_indices at the device step, at steps 0, 1 and 7."""
    from dronerl_amd._native import DroneRLError
    rb, _ = _ring(7, "code", 300)
    _, learner, _ = _learner("b", "code", 8, dict(sample_seed=77))
    for step in range(8):
        if step in (0, 1, 7):
            assert learner.sample_slots(rb.size).cpu().tolist() == O.sample_indices(77, step, 8, rb.size), step
            assert learner.sample_slots(100 + step).cpu().tolist() == O.sample_indices(77, step, 8, 100 + step)
        learner.train(rb)
    assert learner.counters()["step"] == 8
    with pytest.raises(DroneRLError):
        learner.sample_slots(0)


TRAIN_STEPS = 300


@gpu
def test_trained_conv_agent_saves_reloads_and_evaluates(tmp_path):
    """train(..., network_type="conv") end to end: the counters, the three
    checkpoint forms reloaded bit-identical through read_checkpoint, to_qnet
    of the saved file giving the live net's Q bit for bit, the eval table, and
    the agent's mean reward above the random drone's in the same episodes
    (N = 300 steps, the dense test's, already separates them)."""
    from dronerl_amd import EnvParams
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import ConvQNetwork
    from dronerl_amd.train import evaluate, train
    p = EnvParams(n_drones=4, grid_size=9)
    res = train(p, 4096, TRAIN_STEPS, network_type="conv")
    c = res.learner.counters()
    assert c["step"] == TRAIN_STEPS and c["count"] == TRAIN_STEPS and 0.01 <= c["epsilon"] < 1.0
    assert np.isfinite(c["loss"])
    online = [(_host(w), _host(b)) for w, b in res.learner.params("online")]
    for fmt in ("torch", "jax", "torch_agent"):
        path = str(tmp_path / f"agent_{fmt}.safetensors")
        res.learner.save(path, format=fmt)
        ck = read_checkpoint(path)
        assert ck.network_type == "conv" and ck.dense_layers == () and tuple(ck.obs_shape) == (7, 7, 6)
        assert len(ck.conv_layers) == 1 and ck.conv_layers[0]["out_channels"] == 8
        assert np.array_equal(ck.tensors["network.conv2d_1.weight"], online[0][0]), fmt
        assert np.array_equal(ck.tensors["network.conv2d_1.bias"], online[0][1]), fmt
        assert np.array_equal(ck.tensors["network.dense_1.weight"], online[1][0]), fmt
        assert np.array_equal(ck.tensors["network.dense_1.bias"], online[1][1]), fmt
    qnet = to_qnet(read_checkpoint(str(tmp_path / "agent_jax.safetensors")), device="cuda")
    obs = res.env.get_obs(1).reshape(res.env.num_envs, -1)
    live = ConvQNetwork((7, 7, 6), res.net.conv_layers, ())
    live.load(res.net.conv_weights, res.net.conv_biases, res.net.weights, res.net.biases)
    q_live, q_back = torch.empty((res.env.num_envs, 5), device="cuda"), torch.empty((res.env.num_envs, 5), device="cuda")
    live.act(obs, 0.0, q_out=q_live)
    qnet.act(obs, 0.0, q_out=q_back)
    assert torch.equal(q_live, q_back)
    agent, rnd, table = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
    print(f"eval after {TRAIN_STEPS} steps: agent {agent[0]:.4f} +- {agent[1]:.4f}, random {rnd[0]:.4f} +- {rnd[1]:.4f}")
    assert table.shape == (5, 2)
    # (deterministic run; measured: agent -0.1001 +- 0.0171 against random -0.1958 +- 0.0072, a gap of 0.0957;
    # half of it is asserted)
    assert agent[0] > rnd[0] + 0.0478, (agent, rnd)


@gpu
def test_train_main_cli_conv(tmp_path):
    """`python -m dronerl_amd.train --network_type conv`: train, save the jax
    and torch checkpoints, whose metadata reads back, run the final eval."""
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.train import main
    m = main(["--network_type", "conv", "--num_envs", "512", "--num_steps", "60", "--conv_dense_layers", "8",
              "--save_final_checkpoint", "--num_evals", "3", "--num_eval_steps", "200", "--output_dir", str(tmp_path)])
    assert m["obs_per_sec"] > 0 and m["num_gpus"] == 1
    for fmt in ("jax", "torch"):
        ck = read_checkpoint(m[f"checkpoint_{fmt}"])
        assert m[f"checkpoint_{fmt}"].endswith(f"agent_60_steps_{fmt}.safetensors")
        assert ck.network_type == "conv" and ck.dense_layers == (8,) and ck.metadata["conv_dense_layers"] == "(8,)"
        assert ck.metadata["conv_layers"] == "({'kernel_size': 3, 'out_channels': 8, 'padding': 1, 'stride': 1},)"
        assert ck.metadata["dense_layers"] == ("(128, 64)" if fmt == "jax" else "(8,)")
        assert ck.metadata["checkpoint_format"] == fmt
        assert to_qnet(ck, device="cuda").dense_layers == (8,)
    assert -1.0 <= m["eval_reward_mean"] <= 1.0 and -1.0 <= m["random_reward_mean"] <= 1.0
