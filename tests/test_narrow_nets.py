"""Narrow dense Q-networks on the device: hidden widths that are multiples of
8 in [8, 128], the reference's default (16, 16) net (train_jax.py:365) among
them.

The packed act image lays a hidden layer out for its width rounded up to 32
(nt = 2 * ceil(out / 32) 16-row tiles, kt = ceil(in / 32) K-slices, biases
padded to 16 * nt); every pad is an exact zero, written by drl_qnet_pack and
never touched by the learner's in-kernel refresh.  The CPU tests pin the
accepted widths, the packed sizes, the learner's layout and the pack maps on
the padded geometry (a host program, also under ASan + UBSan); the GPU tests
pin the five act paths on padded images (against f32 / bf16 host forwards and,
bit for bit, against the same net embedded in a (32, 32) net with zeros), the
learner against oracle/dqn_learner.py bit for bit, and train() / the command
line end to end on the (16, 16) net.

Tolerances are tests/test_dqn.py's (the widths change no arithmetic: a pad
contributes an exact zero)."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.test_dqn import Q_TOL_BF16, Q_TOL_EXACT, Q_TOL_F32

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

NETS = [(16, 16), (8,), (24, 40, 8), (48, 16), (120, 56), (128, 128, 8)]


def _desc(in_features, hidden, inp=0, precision=0):
    from dronerl_amd.dqn import DrlQnetDesc
    h = list(hidden) + [0] * (3 - len(hidden))
    return DrlQnetDesc(in_features, len(hidden), (ctypes.c_int32 * 3)(*h), 5, precision, inp)


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind
    return _bind(lib())


# ------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("hidden,ok", [(h, True) for h in NETS] +
                         [((4,), False), ((12,), False), ((100,), False), ((136,), False), ((256,), False),
                          ((0,), False)])
@pytest.mark.parametrize("precision", [0, 1])
def test_narrow_desc_validation(hidden, ok, precision):
    L = _lib()
    nb = ctypes.c_int64()
    rc = L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, hidden, precision=precision)), ctypes.byref(nb))
    assert (rc == 0) == ok, L.drl_last_error()
    if ok:
        assert nb.value % 16 == 0
    else:
        assert b"multiples of 8 in [8, 128]" in L.drl_last_error()


def test_narrow_packed_sizes():
    """(294, (16, 16)): layer 0 is 2 tiles x 10 K-slices, layer 1 2 x 1, the
    output layer 1 x 1 (1 KB fragments); biases padded to 32 + 32 + 16 floats;
    the 16-B status vector.  The same bytes as (294, (32, 32)): the physical
    layout is that net's."""
    L = _lib()
    nb, nb32 = ctypes.c_int64(), ctypes.c_int64()
    assert L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, (16, 16))), ctypes.byref(nb)) == 0
    assert nb.value == (2 * 10 + 2 * 1 + 1 * 1) * 1024 + (32 + 32 + 16) * 4 + 16
    assert L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, (32, 32))), ctypes.byref(nb32)) == 0
    assert nb32.value == nb.value
    assert L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, (16, 16), precision=1)), ctypes.byref(nb)) == 0
    assert nb.value == 2 * 23 * 1024 + 320 + 16
    assert L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, (32, 32), precision=1)), ctypes.byref(nb32)) == 0
    assert nb32.value == nb.value
    # a code net's layer 0 has its own K-slice count; the two nets still share one layout
    for inp in (0, 1):
        assert L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, (120, 56), inp, 1)), ctypes.byref(nb)) == 0
        assert L.drl_qnet_packed_bytes(ctypes.byref(_desc(294, (128, 64), inp, 1)), ctypes.byref(nb32)) == 0
        assert nb32.value == nb.value


def test_narrow_dqn_layout():
    """The agent block keeps the logical sizes (in * out rounded to 4 floats);
    layer 0's 16 units are four DQN_TILE-unit tiles per net."""
    from dronerl_amd.dqn import DrlDqnLayout
    L = _lib()
    lay = DrlDqnLayout()
    assert L.drl_dqn_layout_query(ctypes.byref(_desc(294, (16, 16), 1, 1)), 8, ctypes.byref(lay)) == 0, \
        L.drl_last_error()
    # the rule test_dqn_layout_query pins for (128, 64) (its 5 x 64 output layer is 320 floats, not 8 rows):
    # the 5 x 16 output layer is 80 floats, its 5 biases round up to 8
    assert lay.n_params == 294 * 16 + 16 + 16 * 16 + 16 + 5 * 16 + 8
    assert lay.grad_workgroups == 10
    assert 0 < lay.grad_lds_bytes <= 150 * 1024
    assert lay.weight_off[0] == 0 and lay.bias_off[0] == 294 * 16
    assert lay.weight_off[1] == 294 * 16 + 16 and lay.bias_off[1] == lay.weight_off[1] + 16 * 16
    assert lay.weight_off[2] == lay.bias_off[1] + 16 and lay.bias_off[2] == lay.weight_off[2] + 80
    assert (lay.online_off, lay.target_off, lay.m_off, lay.v_off) == tuple(i * 4 * lay.n_params for i in range(4))
    assert lay.counters_off == 16 * lay.n_params and lay.scratch_off == lay.counters_off + 64
    assert lay.bytes % 16 == 0
    for hidden, inp in (((8,), 0), ((48, 16), 0), ((16, 104, 24), 1)):
        assert L.drl_dqn_layout_query(ctypes.byref(_desc(294, hidden, inp, 1)), 32, ctypes.byref(lay)) == 0
        assert lay.grad_workgroups == 2 * (hidden[0] // 4) + 2 and lay.grad_lds_bytes <= 150 * 1024
    assert L.drl_dqn_layout_query(ctypes.byref(_desc(294, (12,), 0, 1)), 8, ctypes.byref(lay)) != 0


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def _build_pack_check(exe, extra):
    subprocess.run([_hipcc(), "-O1", "-std=c++17", *extra, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "narrow_pack_check.cpp")], check=True)


def test_narrow_pack_maps_on_padded_geometry(tmp_path):
    """qnet_pack_slot / qnet_pack_elem on the padded geometry (kt = ceil(in /
    32), nt = 2 * ceil(out / 32), restated in the program): the property the
    new layout relies on.  The two maps are unchanged code, so this passes on
    the multiples-of-32 build too; what ties the program's geometry to
    qnet_layout is test_narrow_packed_sizes, and the GPU embedding test."""
    exe = str(tmp_path / "narrow_pack_check")
    _build_pack_check(exe, [])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout


CLANG = "/opt/rocm/llvm/bin/clang"


def test_narrow_pack_maps_clean_under_asan_ubsan(tmp_path):
    """The same stand-alone host program with its host code under ASan + UBSan
    (linked against the sanitizer runtime: nothing preloaded).  Skipped only
    where the compiler ships no ASan runtime (probed before anything is
    built, as tests/test_sanitizers.py does); a build that fails fails."""
    _hipcc()
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    rt = subprocess.run([CLANG, "-print-file-name=libclang_rt.asan-x86_64.a"], capture_output=True, text=True,
                        check=True).stdout.strip()
    if not os.path.exists(rt):
        pytest.skip("clang ASan runtime not found")
    exe = str(tmp_path / "narrow_pack_check_san")
    _build_pack_check(exe, ["-g", "--offload-host-only", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


# ------------------------------------------------------------------- GPU ---
@functools.lru_cache(maxsize=None)
def _inputs(E, radius):
    """C3-shape observations and drone 0's policy code after a few steps
    (computed once per shape and shared; never written)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=radius), E)
    env.reset(seed=E + radius)
    code = env.new_code()
    for t in range(6):
        _, _, obs = env.step(env.synth_actions(seed=2, step=t), obs_k=1, code=code)
    env.check_errors()
    return obs.reshape(E, -1).contiguous().clone(), code.clone()


def _net(in_features, hidden, seed, precision="f32", inp="obs"):
    from dronerl_amd.dqn import QNetwork
    net = QNetwork(in_features, hidden, generator=torch.Generator().manual_seed(seed), precision=precision, input=inp)
    gb = torch.Generator(device="cuda").manual_seed(seed + 1)
    for b in net.biases:
        b.normal_(0, 0.1, generator=gb)
    net.packed.fill_(0x7F7F7F7F)  # (a pad the pack leaves unwritten would be a large finite weight)
    net.pack()
    return net


def _f32_forward(net, x):
    ref = x.cpu()
    for i, (w, b) in enumerate(zip(net.weights, net.biases)):
        ref = ref @ w.cpu().t() + b.cpu()
        if i < len(net.weights) - 1:
            ref = torch.relu(ref)
    return ref


def _check_f32(net, inp, x):
    """Every env's Q within Q_TOL_EXACT * (1 + max |Q_ref|) of the f32 host
    forward; the action is the first argmax of the kernel's own Q, and its
    reference Q is within twice that tolerance of the reference maximum."""
    E = x.shape[0]
    q = torch.empty((E, 5), device="cuda")
    a = net.act(inp, epsilon=0.0, q_out=q)
    net.check_errors()
    ref = _f32_forward(net, x)
    tol = Q_TOL_EXACT * (1.0 + ref.abs().amax(dim=1))
    err = (q.cpu() - ref).abs().amax(dim=1)
    print(f"max |Q - Q_ref| / tol = {(err / tol).max().item():.3f}")
    assert torch.all(err <= tol), (err / tol).max().item()
    act = a[:, 0].cpu().long()
    assert torch.equal(act, torch.argmax(q.cpu(), dim=1))
    assert torch.all(ref.gather(1, act[:, None])[:, 0] >= ref.amax(dim=1) - 2 * tol)


@gpu
@pytest.mark.parametrize("hidden,radius", [(h, 3) for h in NETS] + [((16,), 4)])
@pytest.mark.parametrize("E", [31, 1000])
def test_narrow_f32_obs_act_matches_f32_forward(hidden, radius, E):
    x, _ = _inputs(E, radius)
    _check_f32(_net(x.shape[1], hidden, seed=len(hidden) * 1000 + E + hidden[0]), x, x)


@gpu
@pytest.mark.parametrize("hidden,radius", [(h, 3) for h in NETS] + [((16,), 4)])
def test_narrow_bf16_obs_act(hidden, radius):
    """As test_qnet_greedy_matches_torch_reference's Q checks."""
    E = 1000
    x, _ = _inputs(E, radius)
    net = _net(x.shape[1], hidden, seed=len(hidden) * 1000 + hidden[0], precision="bf16")
    q = torch.empty((E, 5), device="cuda")
    a = net.act(x, epsilon=0.0, q_out=q)
    ref = net.reference_q(x, bf16_operands=True)
    ref32 = net.reference_q(x)
    assert torch.all((q - ref).abs() <= Q_TOL_BF16 * (1 + ref.abs())), (q - ref).abs().max()
    assert torch.all((q - ref32).abs() <= Q_TOL_F32 * (1 + ref32.abs())), (q - ref32).abs().max()
    assert torch.equal(a[:, 0].long(), torch.argmax(q, dim=1))


def _embed(net, wide):
    """net's parameters in a `wide`-hidden net: zero extra rows, columns and biases."""
    sizes_n = [net.in_features, *net.hidden, net.n_actions]
    sizes_w = [net.in_features, *wide, net.n_actions]
    ws, bs = [], []
    for l, (w, b) in enumerate(zip(net.weights, net.biases)):
        W = torch.zeros((sizes_w[l + 1], sizes_w[l]), device=w.device)
        B = torch.zeros(sizes_w[l + 1], device=w.device)
        W[:sizes_n[l + 1], :sizes_n[l]] = w
        B[:sizes_n[l + 1]] = b
        ws.append(W)
        bs.append(B)
    return ws, bs


@gpu
@pytest.mark.parametrize("path", ["bf16", "f32", "code"])
@pytest.mark.parametrize("hidden", [(16, 16), (24, 8)])
def test_narrow_net_equals_its_zero_embedding(hidden, path):
    """A narrow net and the same net embedded in a (32, 32) net (zero extra
    rows, columns and biases) share one physical layout: the packed images are
    byte-identical, and Q and the actions are bit-identical on every act path.
    A pad that is not an exact zero, or that an act reads as anything else,
    shows here.  (The one-tile layer-0 instance the A/B tried was not kept,
    profiles/narrow_nets/act_ab.txt, so there is no instance knob to turn.)"""
    from dronerl_amd.dqn import QNetwork
    E = 1000
    x, code = _inputs(E, 3)
    precision, inp = ("bf16", "obs") if path == "bf16" else ("f32", "code" if path == "code" else "obs")
    narrow = _net(x.shape[1], hidden, seed=hidden[0] + len(path), precision=precision, inp=inp)
    wide = QNetwork(x.shape[1], (32, 32), precision=precision, input=inp)
    wide.packed.fill_(0x7F7F7F7F)
    wide.load(*_embed(narrow, (32, 32)))
    assert torch.equal(narrow.packed, wide.packed)
    src = code if inp == "code" else x
    qn, qw = torch.empty((E, 5), device="cuda"), torch.empty((E, 5), device="cuda")
    an = narrow.act(src, epsilon=0.25, seed=3, step=1, q_out=qn)
    aw = wide.act(src, epsilon=0.25, seed=3, step=1, q_out=qw)
    narrow.check_errors()
    wide.check_errors()
    assert torch.equal(qn, qw) and torch.equal(an, aw)
    assert float(qn.abs().max()) > 0 and bool(torch.isfinite(qn).all())


@gpu
@pytest.mark.parametrize("hidden,kernel", [((16, 16), "auto"), ((48, 16), "auto"), ((120, 56), "auto"),
                                           ((120, 56), "code2")])
def test_narrow_code_act_matches_f32_forward(hidden, kernel, monkeypatch):
    """(120, 56) lands on the specialised 128 -> 64 instances through its pads
    (drl_qnet_act_code4_kernel; DRL_QN_CODE=2: drl_qnet_act_code2_kernel)."""
    if kernel == "code2":
        monkeypatch.setenv("DRL_QN_CODE", "2")
    x, code = _inputs(1000, 3)
    _check_f32(_net(x.shape[1], hidden, seed=hidden[0] + 7, inp="code"), code, x)


@gpu
@pytest.mark.parametrize("sizes,inp,hp_kw,E,cap", [
    ((294, 16, 16, 5), "code", dict(batch=8, num_steps=1000), 64, 300),                      # train_jax defaults
    ((294, 8, 5), "obs", dict(batch=1), 16, 100),
    ((294, 48, 16, 5), "obs", dict(batch=32, tau=0.6, target_update_interval=3), 50, 257),
    ((294, 16, 104, 24, 5), "code", dict(batch=8), 32, 200),
    # a later hidden layer of 8 units: the tails run it one output per lane quad (dq_forward's lo <= 8 branch,
    # dq_mm1), until now the output layer's path only; the same four partial sums, combined alike
    ((294, 16, 8, 5), "code", dict(batch=8), 32, 200),
    ((294, 24, 40, 8, 5), "obs", dict(batch=4, tau=0.5, target_update_interval=2), 32, 200),
])
def test_narrow_learner_matches_oracle_bit_exact(sizes, inp, hp_kw, E, cap):
    """test_learner_matches_oracle_bit_exact's loop on narrow nets: parameters,
    target, moments, loss and counters equal oracle/dqn_learner.py bit for bit
    after each of 40 steps; at the end the image the learner refreshed acts
    exactly as a fresh pack of its online parameters."""
    from oracle import dqn_learner as O
    from dronerl_amd.dqn import QNetwork
    from tests.test_dqn_learner import _host, _learner_setup, assert_same, oracle_hparams, state_from_learner
    env, net, learner, rb, hp = _learner_setup(sizes, inp, hp_kw, E=E, cap=cap)
    st = state_from_learner(learner)
    ohp = oracle_hparams(hp)
    W = 7
    cur = env.new_code() if inp == "code" else torch.empty((E, 1, W, W, 6), device="cuda")
    nxt = env.new_code() if inp == "code" else torch.empty((E, 1, W, W, 6), device="cuda")
    if inp == "code":
        env.get_code(out=cur)
    else:
        env.get_obs(1, out=cur)
    acts = torch.empty((E, 8), dtype=torch.int32, device="cuda")
    trained = 0
    for t in range(40):
        x = cur if inp == "code" else cur.reshape(E, -1)
        assert np.float32(float(learner.epsilon.item())) == st.epsilon
        net.act(x, learner.epsilon, seed=3, step=t, actions=acts, synth=(5, t))
        if inp == "code":
            r, d = env.step(acts, code=nxt)
        else:
            r, d, _ = env.step(acts, obs_k=1, obs=nxt)
        rb.add_many(cur, acts, r, nxt, d)
        info = O.learner_step(st, ohp, _host(rb.obs), _host(rb.next_obs), _host(rb.actions), _host(rb.rewards),
                              _host(rb.dones), rb.size, W if inp == "code" else 0)
        trained += info["trained"]
        learner.train(rb)
        torch.cuda.synchronize()
        assert_same(learner, st, t)
        cur, nxt = nxt, cur
    net.check_errors()
    env.check_errors()
    learner.check_errors()
    assert trained >= 30
    x = cur if inp == "code" else cur.reshape(E, -1)
    fresh = QNetwork(sizes[0], sizes[1:-1], precision="f32", input=inp)
    fresh.packed.fill_(0x7F7F7F7F)
    fresh.load(*zip(*learner.params("online")))
    q0, q1 = torch.empty((E, 5), device="cuda"), torch.empty((E, 5), device="cuda")
    a0 = net.act(x, 0.0, q_out=q0)
    a1 = fresh.act(x, 0.0, q_out=q1)
    assert torch.equal(q0, q1) and torch.equal(a0, a1)
    assert torch.equal(net.packed, fresh.packed)  # (the refresh wrote no pad, the pack wrote every pad as zero)


@gpu
def test_narrow_train_end_to_end(tmp_path):
    """train() on the reference's default (16, 16) net, saved in the three
    formats and reloaded onto the act kernel; then the command line."""
    from dronerl_amd import EnvParams
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import QNetwork
    from dronerl_amd.train import main, train
    res = train(EnvParams(n_drones=4, grid_size=9), 512, 60, hidden=(16, 16))
    c = res.learner.counters()
    assert c["step"] == 60 and c["count"] == 60
    obs = res.env.get_obs(1).reshape(res.env.num_envs, -1)
    live = QNetwork(294, (16, 16), precision="f32")
    live.load(*zip(*res.learner.params("online")))
    q_live = torch.empty((res.env.num_envs, 5), device="cuda")
    live.act(obs, 0.0, q_out=q_live)
    for fmt in ("torch", "jax", "torch_agent"):
        path = str(tmp_path / f"agent_{fmt}.safetensors")
        res.learner.save(path, format=fmt)
        ck = read_checkpoint(path)
        assert ck.dense_layers == (16, 16) and tuple(ck.obs_shape) == (7, 7, 6)
        q_back = torch.empty_like(q_live)
        to_qnet(ck, device="cuda").act(obs, 0.0, q_out=q_back)
        assert torch.equal(q_live, q_back), fmt
    m = main(["--num_envs", "512", "--num_steps", "60", "--hidden_layers", "16", "16", "--save_final_checkpoint",
              "--num_evals", "2", "--num_eval_steps", "200", "--output_dir", str(tmp_path)])
    assert m["obs_per_sec"] > 0
    for fmt in ("jax", "torch"):
        assert read_checkpoint(m[f"checkpoint_{fmt}"]).dense_layers == (16, 16)
    assert -1.0 <= m["eval_reward_mean"] <= 1.0
