"""Dense Q-networks with hidden widths up to 256 (run_jax_sweep.py trains
hidden_layers = (256, 128, 64)): drl_widenet_* (dronerl_amd/csrc/widenet/),
dqn.WideQNetwork, dqn.WideDQNLearner, dqn.make_learner, checkpoint.to_qnet and
`python -m dronerl_amd.train --hidden_layers 256 128 64`.

Reference: jax_impl/agents/dqn.py:47-63 DenseQNetwork and :132-146 act,
train_jax.py:38-115, run_jax_sweep.py:26.

The act: Q against an f32 host forward and an f64 one by tests/test_dqn.py's
rule (Q_TOL_EXACT = 1e-5 relative to 1 + max|Q_ref| of the row; a CPU
emulation of the hi/lo split gives at most 1.4e-6 on these shapes), the
exploration stream against QNetwork.act's, code input against obs input bit
for bit.  The learner: oracle/dqn_learner.py BIT FOR BIT after every step, as
tests/test_large_batch_learner.py checks the chain it shares."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import dqn_learner as O

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SETS = ("online", "target", "m", "v")
Q_TOL_EXACT = 1e-5  # tests/test_dqn.py's


# ------------------------------------------------------------ C ABI (CPU) ---
def _desc(in_features, hidden, inp=0, n_actions=5):
    from dronerl_amd.dqn import DrlWidenetDesc
    h = list(hidden) + [0] * (3 - len(hidden))
    return DrlWidenetDesc(in_features, len(hidden), (ctypes.c_int32 * 3)(*h[:3]), n_actions, inp)


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind, _bind_widenet
    return _bind_widenet(_bind(lib()))


def test_widenet_descriptor_validation():
    """drl_widenet_packed_bytes accepts widths 8..256 (narrow nets too) and
    refuses every field outside its limits by name (host only)."""
    L = _lib()
    nb = ctypes.c_int64()

    def ok(d):
        return L.drl_widenet_packed_bytes(ctypes.byref(d), ctypes.byref(nb)) == 0

    for hidden in ((8,), (136,), (256,), (256, 128, 64), (16, 16), (256, 256, 256)):
        assert ok(_desc(294, hidden)), (hidden, L.drl_last_error())
        assert nb.value > 0 and nb.value % 16 == 0
    # the sweep net: hi + lo fragments of 16x10, 8x8, 4x4 and 1x2 (unit tiles x K-slices), the biases, the status
    assert ok(_desc(294, (256, 128, 64)))
    assert nb.value == 2 * (160 + 64 + 16 + 2) * 1024 + (256 + 128 + 64 + 16) * 4 + 16
    assert ok(_desc(512, (256, 256, 256), n_actions=8)) and 1.0e6 < nb.value < 1.2e6  # the widest: ~1.1 MB
    for w in (4, 12, 264, 0):
        assert not ok(_desc(294, (w,))) and b"hidden widths" in L.drl_last_error(), w
        assert not ok(_desc(294, (256, w))) and b"hidden widths" in L.drl_last_error(), w
    assert b"[8, 256]" in L.drl_last_error()
    for nh in (0, 4):
        d = _desc(294, (64,))
        d.n_hidden = nh
        assert not ok(d) and b"n_hidden" in L.drl_last_error(), nh
    for a in (9, 0):
        assert not ok(_desc(294, (64,), n_actions=a)) and b"n_actions" in L.drl_last_error()
    for f in (0, 514, 293):
        assert not ok(_desc(f, (64,))) and b"in_features" in L.drl_last_error(), f
    for f in (292, 6, 512):  # a code net: W*W*6 for W in 5, 7, 9 only
        assert not ok(_desc(f, (64,), inp=1)) and b"policy-code" in L.drl_last_error(), f
    for f in (150, 294, 486):
        assert ok(_desc(f, (256,), inp=1)), f
    assert not ok(_desc(294, (64,), inp=2)) and b"input" in L.drl_last_error()
    assert L.drl_widenet_packed_bytes(None, ctypes.byref(nb)) != 0 and b"NULL" in L.drl_last_error()
    assert L.drl_widenet_packed_bytes(ctypes.byref(_desc(294, (64,))), None) != 0 and b"bytes is NULL" in L.drl_last_error()
    # the existing families keep their limit
    from dronerl_amd.dqn import DrlDqnLayout, DrlQnetDesc
    q = DrlQnetDesc(294, 1, (ctypes.c_int32 * 3)(256, 0, 0), 5, 1, 0)
    assert L.drl_qnet_packed_bytes(ctypes.byref(q), ctypes.byref(nb)) != 0 and b"[8, 128]" in L.drl_last_error()
    assert L.drl_dqn_large_layout_query(ctypes.byref(q), 8, ctypes.byref(DrlDqnLayout())) != 0


def test_widenet_calls_validate_before_device_work():
    """Every pointer, alignment, stride, batch and row kind is checked before
    any device work (no GPU needed); the learner's layout is the large-batch
    learner's at the widths both take."""
    from dronerl_amd.dqn import DQNHParams, DrlDqnLayout, DrlQnetDesc, DrlReplay
    L = _lib()
    vp = ctypes.c_void_p
    d, dc = _desc(294, (256, 128, 64)), _desc(294, (256, 128, 64), 1)
    P = vp(1 << 20)

    def act(desc=d, packed=P, x=P, E=10, stride=294, eps=None, acts=P, astride=1):
        return L.drl_widenet_act(ctypes.byref(desc), packed, x, E, stride, 0.0, eps, 0, 0, 0, acts, astride, None, None,
                                 None)
    assert act(E=0) == 0  # (nothing to do)
    assert act(E=-1) != 0 and b"num_envs" in L.drl_last_error()
    assert act(packed=None) != 0 and b"non-NULL" in L.drl_last_error()
    assert act(x=None) != 0 and b"non-NULL" in L.drl_last_error()
    assert act(acts=None) != 0 and b"non-NULL" in L.drl_last_error()
    assert act(packed=vp((1 << 20) + 8)) != 0 and b"16-byte" in L.drl_last_error()
    assert act(x=vp((1 << 20) + 4)) != 0 and b"8-byte" in L.drl_last_error()
    assert act(stride=295) != 0 and b"8-byte" in L.drl_last_error()
    assert act(stride=292) != 0 and b"obs_stride" in L.drl_last_error()
    assert act(desc=dc, x=vp((1 << 20) + 8)) != 0 and b"policy code" in L.drl_last_error()
    assert act(eps=vp((1 << 20) + 2)) != 0 and b"d_epsilon" in L.drl_last_error()
    assert act(astride=0) != 0 and b"action_stride" in L.drl_last_error()
    bad = _desc(294, (264,))
    assert act(desc=bad) != 0 and b"hidden widths" in L.drl_last_error()
    pp = (vp * 4)(P, P, P, P)
    assert L.drl_widenet_pack(ctypes.byref(d), None, pp, P, None) != 0 and b"non-NULL" in L.drl_last_error()
    assert L.drl_widenet_pack(ctypes.byref(d), pp, pp, vp((1 << 20) + 4), None) != 0 and b"16-byte" in L.drl_last_error()
    assert L.drl_widenet_pack(ctypes.byref(d), (vp * 4)(P, None, P, P), pp, P, None) != 0 and b"NULL" in L.drl_last_error()
    # the learner
    hp = DQNHParams(batch=1024).c()
    good = DrlReplay(5000, 294, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)

    def train(desc=d, h=hp, agent=P, packed=vp(1 << 21), r=good, size=100):
        return L.drl_widenet_dqn_train(ctypes.byref(desc), None if h is None else ctypes.byref(h), agent, packed,
                                       None if r is None else ctypes.byref(r), size, None)
    assert train(h=None) != 0 and b"hparams is NULL" in L.drl_last_error()
    assert train(agent=None) != 0 and b"agent block" in L.drl_last_error()
    assert train(packed=vp((1 << 21) + 4)) != 0 and b"16-byte" in L.drl_last_error()
    assert train(r=None) != 0 and b"replay" in L.drl_last_error()
    assert train(size=5001) != 0 and b"size" in L.drl_last_error()
    assert train(r=DrlReplay(5000, 292, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20)) != 0 and b"obs_floats" in L.drl_last_error()
    assert train(desc=dc) != 0 and b"policy code" in L.drl_last_error()  # f32 rows for a code net
    for batch in (0, 4097):
        assert train(h=DQNHParams(batch=batch).c()) != 0 and b"batch must be in [1, 4096]" in L.drl_last_error()
    assert train(h=DQNHParams(batch=8, beta2=1.0).c()) != 0 and b"beta1" in L.drl_last_error()
    assert train(desc=bad) != 0 and b"hidden widths" in L.drl_last_error()
    assert L.drl_widenet_dqn_init(ctypes.byref(d), 8, None, 1.0, None) != 0 and b"agent block" in L.drl_last_error()
    assert L.drl_widenet_dqn_init(ctypes.byref(d), 4097, P, 1.0, None) != 0 and b"batch" in L.drl_last_error()
    assert L.drl_widenet_dqn_sample_rows(ctypes.byref(d), ctypes.byref(hp), P, 100, None, None) != 0
    assert b"d_slots" in L.drl_last_error()
    assert L.drl_widenet_dqn_sample_rows(ctypes.byref(d), ctypes.byref(hp), P, 0, P, None) != 0 and b"size" in L.drl_last_error()
    assert L.drl_widenet_dqn_sample_rows(ctypes.byref(d), None, P, 10, P, None) != 0 and b"hparams" in L.drl_last_error()
    lay = DrlDqnLayout()
    assert L.drl_widenet_dqn_layout_query(ctypes.byref(d), 8, None) != 0 and b"layout is NULL" in L.drl_last_error()
    for batch in (1, 65, 4096):
        assert L.drl_widenet_dqn_layout_query(ctypes.byref(d), batch, ctypes.byref(lay)) == 0, L.drl_last_error()
        marks = [lay.online_off, lay.target_off, lay.m_off, lay.v_off, lay.counters_off, lay.scratch_off, lay.bytes]
        assert lay.n_params >= 294 * 256 + 256 * 128 + 128 * 64 + 64 * 5 + 256 + 128 + 64 + 5
        assert marks[0] == 0 and all(m % 16 == 0 for m in marks) and marks == sorted(marks)
        assert marks[1] - marks[0] == 4 * lay.n_params
    wide, large = DrlDqnLayout(), DrlDqnLayout()
    q = DrlQnetDesc(294, 2, (ctypes.c_int32 * 3)(128, 64, 0), 5, 1, 1)
    assert L.drl_widenet_dqn_layout_query(ctypes.byref(_desc(294, (128, 64), 1)), 300, ctypes.byref(wide)) == 0
    assert L.drl_dqn_large_layout_query(ctypes.byref(q), 300, ctypes.byref(large)) == 0
    assert bytes(wide) == bytes(large)


def test_widenet_layout_places_every_image_element_once(tmp_path):
    """tests/native/widenet_layout_check.cpp, a stand-alone program under the
    address and undefined-behaviour sanitizers: every (layer, unit, input,
    piece) has its own in-bounds element of the image and every other element
    is a pad, every LDS word of the act's plan is inside the workgroup's
    allocation (at most 160 KB), and the learner's plan takes width 256 at
    batches 1, 65 and 4096 and refuses 264.  Nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "widenet_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "widenet_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_python_routing_without_a_device(monkeypatch):
    """to_qnet's class by the checkpoint's widths (128: QNetwork; 136 and 256:
    WideQNetwork; 264 refused), make_learner's dispatch on the net's type, the
    command line and the sharding refusal -- the classes stubbed: no device."""
    from dronerl_amd import checkpoint, dqn, train
    made = []

    class _Stub:
        def __init__(self, name):
            self.name = name

        def __call__(self, in_features, hidden, n_actions, **kw):
            made.append((self.name, in_features, tuple(hidden), n_actions, kw))
            return self

        def load(self, ws, bs):
            made.append(("load", self.name, [tuple(w.shape) for w in ws]))

    real_wide = dqn.WideQNetwork
    monkeypatch.setattr(dqn, "QNetwork", _Stub("QNetwork"))
    monkeypatch.setattr(dqn, "WideQNetwork", _Stub("WideQNetwork"))

    def ck(hidden):
        sizes = [150, *hidden, 5]
        t = {}
        for i in range(len(sizes) - 1):
            t[f"network.dense_{i + 1}.weight"] = np.zeros((sizes[i + 1], sizes[i]), np.float32)
            t[f"network.dense_{i + 1}.bias"] = np.zeros(sizes[i + 1], np.float32)
        return checkpoint.Checkpoint("dense", (5, 5, 6), (5,), tuple(hidden), (), t)

    for hidden, want in (((128,), "QNetwork"), ((128, 64), "QNetwork"), ((16, 16), "QNetwork"), ((136,), "WideQNetwork"),
                         ((256,), "WideQNetwork"), ((256, 128, 64), "WideQNetwork"), ((64, 136), "WideQNetwork")):
        made.clear()
        assert checkpoint.to_qnet(ck(hidden), device="cpu").name == want
        assert made[0][:4] == (want, 150, hidden, 5) and made[1][:2] == ("load", want), made
    assert made[0][4] == {"device": "cpu", "input": "obs"}
    checkpoint.to_qnet(ck((256,)), device="cpu", input="code")
    assert made[-2][4]["input"] == "code"
    for hidden in ((264,), (256, 264), (12,), (), (64, 64, 64, 64)):
        with pytest.raises(ValueError, match="unsupported"):
            checkpoint.to_qnet(ck(hidden), device="cpu")
    with pytest.raises(ValueError, match="input='code'"):  # (as before: a narrow dense checkpoint)
        checkpoint.to_qnet(ck((128,)), device="cpu", input="code")
    assert dqn.is_wide((256, 128, 64)) and dqn.is_wide((64, 136)) and not dqn.is_wide((128, 128, 128))
    # make_learner: by the net's type first, then by the batch
    monkeypatch.setattr(dqn, "WideQNetwork", real_wide)
    learners = []
    for name in ("DQNLearner", "LargeBatchDQNLearner", "WideDQNLearner"):
        monkeypatch.setattr(dqn, name, lambda net, hp, _n=name, **kw: learners.append((_n, hp.batch, kw)) or _n)
    wide = object.__new__(real_wide)
    for batch in (1, 8, 64, 65, 4096):
        assert dqn.make_learner(wide, dqn.DQNHParams(batch=batch), generator=None) == "WideDQNLearner"
        assert learners[-1] == ("WideDQNLearner", batch, {"generator": None})
    assert dqn.make_learner(wide) == "WideDQNLearner"
    assert dqn.make_learner(object(), dqn.DQNHParams(batch=8)) == "DQNLearner"
    assert dqn.make_learner(object(), dqn.DQNHParams(batch=65)) == "LargeBatchDQNLearner"
    # the command line
    a = train.parse_args(["--hidden_layers", "256", "128", "64"])
    assert tuple(a.hidden_layers) == (256, 128, 64) and a.network_type == "dense" and not a.use_sharding
    with pytest.raises(ValueError, match="wider than 128"):
        train.parse_args(["--hidden_layers", "256", "128", "64", "--use_sharding", "--num_envs", "8"])
    train.parse_args(["--hidden_layers", "128", "64", "--use_sharding", "--num_envs", "8"])  # (narrow: as before)
    assert "wider than 128" in train.WIDE_SHARDING_REFUSAL
    from dronerl_amd import EnvParams
    with pytest.raises(ValueError, match="wider than 128"):  # refused before anything touches a device
        train.train(EnvParams(), 8, 4, hidden=(256, 128, 64), world=2, rank=0)


# Every __global__ kernel under csrc/widenet/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_widenet_pack_kernel": "test_wide_nets.py::test_wide_learner_matches_oracle_bit_exact",
    "drl_widenet_act_kernel": "test_wide_nets.py::test_wide_q_matches_f32_and_f64_forward",
}


def test_every_widenet_kernel_has_a_gpu_test():
    import glob
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "widenet", "*.hip")):
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
        assert re.search(rf"^@gpu\n(?:@pytest[^\n]*\n)*def {test}\(", text, re.M), (kern, ref)


# ------------------------------------------------------------------- GPU ---
E_MAX = 1000
# 1, around one MFMA tile, around a workgroup's envs (32 at two tiles per pass, 64 at four), many workgroups
ENV_COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, E_MAX)


def _host(t):
    return t.detach().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _windows(radius):
    """E_MAX env windows [E, W*W*6] and their policy codes (shared, read only)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=radius), E_MAX)
    env.reset(seed=radius)
    for t in range(5):
        env.step(env.synth_actions(seed=1, step=t))
    code = env.new_code()
    obs = env.get_obs(1, code=code).reshape(E_MAX, -1).contiguous()
    torch.cuda.synchronize()
    return obs, code


@functools.lru_cache(maxsize=None)
def _rows(source, n):
    """E_MAX input rows (shared, read only): env windows or dense randn rows."""
    if source == "window":
        return _windows({150: 2, 294: 3, 486: 4}[n])[0]
    return torch.randn((E_MAX, n), generator=torch.Generator().manual_seed(n)).cuda()


def _wide(in_features, hidden, n_actions=5, seed=0, inp="obs"):
    from dronerl_amd.dqn import WideQNetwork
    net = WideQNetwork(in_features, hidden, n_actions=n_actions, generator=torch.Generator().manual_seed(seed), input=inp)
    gb = torch.Generator(device="cuda").manual_seed(seed + 7)
    for b in net.biases:
        b.normal_(0, 0.1, generator=gb)
    net.pack()
    return net


def _host_forwards(net, x):
    """An f32 forward on the host (plain IEEE f32 matmuls) and an f64 one."""
    ref32, ref64 = x.cpu().clone(), x.cpu().double()
    for i, (w, b) in enumerate(zip(net.weights, net.biases)):
        ref32 = ref32 @ w.cpu().t() + b.cpu()
        ref64 = ref64 @ w.cpu().double().t() + b.cpu().double()
        if i < len(net.weights) - 1:
            ref32, ref64 = torch.relu(ref32), torch.relu(ref64)
    return ref32, ref64


Q_CASES = [
    # hidden, input rows, in_features, actions
    ((256, 128, 64), "window", 294, 5),
    ((256, 128, 64), "randn", 294, 5),
    ((256, 128, 64), "randn", 150, 1),
    ((136,), "window", 150, 8),
    ((136,), "randn", 512, 5),
    ((256, 256, 256), "window", 486, 5),
    ((256, 256, 256), "randn", 512, 8),
    ((256, 256, 256), "randn", 6, 5),
    ((8,), "randn", 6, 1),
    ((8,), "window", 294, 8),
    ((16, 16), "randn", 510, 5),
    ((16, 16), "window", 150, 5),
]


Q_IDS = ["-".join(map(str, (c[2], *c[0], c[3]))) + "-" + c[1] for c in Q_CASES]


@gpu
@pytest.mark.parametrize("hidden,source,n_in,n_actions", Q_CASES, ids=Q_IDS)
def test_wide_q_matches_f32_and_f64_forward(hidden, source, n_in, n_actions):
    """drl_widenet_act's Q against an f32 host forward and an f64 one within
    Q_TOL_EXACT of 1 + max|Q_ref| of the row, and the greedy action by
    tests/test_dqn.py's rule (the f32 argmax wherever the top two Q values are
    further apart than 2 tol; always the first argmax of its own Q), at every
    env count of ENV_COUNTS; nothing is written behind the E rows of q and of
    the actions or into the other action columns; rows of a wider stride inside
    a NaN-filled buffer give the packed rows' Q bit for bit."""
    x = _rows(source, n_in)
    net = _wide(n_in, hidden, n_actions, seed=len(hidden) * 1000 + n_in)
    ref32, ref64 = _host_forwards(net, x)
    scale = 1.0 + ref32.abs().amax(dim=1, keepdim=True)
    worst = 0.0
    for E in ENV_COUNTS:
        q = torch.full((E + 1, n_actions), -777.0, device="cuda")
        acts = torch.full((E + 1, 3), -7, dtype=torch.int32, device="cuda")
        net.act(x[:E], 0.0, actions=acts[:E], q_out=q[:E])
        qc, ac = q.cpu(), acts.cpu()
        assert torch.all(qc[E] == -777.0) and torch.all(ac[E] == -7) and torch.all(ac[:E, 1:] == -7), E
        qc, act = qc[:E], ac[:E, 0].long()
        err = ((qc - ref32[:E]).abs() / scale[:E]).max().item()
        err64 = ((qc.double() - ref64[:E]).abs() / scale[:E].double()).max().item()
        worst = max(worst, err, err64)
        assert err <= Q_TOL_EXACT and err64 <= Q_TOL_EXACT, (E, err, err64)
        assert torch.equal(act, torch.argmax(qc, dim=1)), E  # the first argmax of its own Q
        if n_actions > 1:
            top2 = torch.topk(ref32[:E], 2, dim=1).values
            tol = 2 * Q_TOL_EXACT * scale[:E, 0]
            clear = (top2[:, 0] - top2[:, 1]) > tol
            assert torch.equal(act[clear], torch.argmax(ref32[:E], dim=1)[clear]), E
            assert torch.all(ref32[:E].gather(1, act[:, None])[:, 0] >= top2[:, 0] - tol), E
            if E == E_MAX:
                assert clear.float().mean() > 0.99
    print(f"wide act {n_in}-{hidden}-{n_actions} {source}: max relative error {worst:.3g}")
    # rows of stride in_features + 10 inside a NaN-filled buffer
    E = 65
    q0, q1 = torch.empty((E, n_actions), device="cuda"), torch.empty((E, n_actions), device="cuda")
    buf = torch.full((E, n_in + 10), float("nan"), device="cuda")
    buf[:, :n_in] = x[:E]
    a0 = net.act(x[:E], 0.0, q_out=q0)
    a1 = net.act(buf, 0.0, q_out=q1)
    assert torch.equal(q0.view(torch.int32), q1.view(torch.int32)) and torch.equal(a0, a1)
    net.check_errors()


@gpu
def test_wide_exploration_stream_is_qnetworks():
    """With epsilon = 1 every env explores: the actions are QNetwork.act's for
    the same (seed, step, env_offset) on a net both accept; with a device
    epsilon tensor the result equals the host-float call; an [E, n] actions
    tensor keeps its other columns."""
    from dronerl_amd.dqn import QNetwork
    x = _rows("window", 294)
    wide = _wide(294, (128, 64), seed=3)
    narrow = QNetwork(294, (128, 64), precision="f32")
    narrow.load(wide.weights, wide.biases)
    for E, seed, step, off in ((E_MAX, 11, 0, 0), (65, 2**63 + 5, 123456, 7_000_000), (17, 0, 3, 1)):
        a = wide.act(x[:E], 1.0, seed=seed, step=step, env_offset=off)
        b = narrow.act(x[:E], 1.0, seed=seed, step=step, env_offset=off)
        assert torch.equal(a, b), (E, seed)
    assert len(set(wide.act(x, 1.0, seed=11)[:, 0].tolist())) == 5
    for eps in (0.0, 0.3, 1.0):
        qa, qb = torch.empty((E_MAX, 5), device="cuda"), torch.empty((E_MAX, 5), device="cuda")
        a = wide.act(x, eps, seed=4, step=9, env_offset=100, q_out=qa)
        b = wide.act(x, torch.tensor([eps], device="cuda"), seed=4, step=9, env_offset=100, q_out=qb)
        assert torch.equal(a, b) and torch.equal(qa, qb), eps
    greedy, mixed = wide.act(x, 0.0, seed=4, step=9), wide.act(x, 0.3, seed=4, step=9)
    frac = (greedy != mixed).float().mean().item()
    assert 0.15 < frac < 0.33  # ~0.3 * 4 / 5 of the envs take another action
    wide.check_errors()


@gpu
@pytest.mark.parametrize("hidden", [(128, 64), (16, 16)])
def test_wide_act_agrees_with_the_narrow_f32_act(hidden):
    """A net both families accept: the wide path's Q is within 2 Q_TOL_EXACT
    (each is within Q_TOL_EXACT of the f32 forward) of QNetwork(precision=
    "f32")'s on the same rows, relative to 1 + max|Q| of the row."""
    from dronerl_amd.dqn import QNetwork
    x = _rows("window", 294)
    wide = _wide(294, hidden, seed=5)
    narrow = QNetwork(294, hidden, precision="f32")
    narrow.load(wide.weights, wide.biases)
    qw, qn = torch.empty((E_MAX, 5), device="cuda"), torch.empty((E_MAX, 5), device="cuda")
    wide.act(x, 0.0, q_out=qw)
    narrow.act(x, 0.0, q_out=qn)
    scale = 1.0 + qn.abs().amax(dim=1, keepdim=True)
    err = ((qw - qn).abs() / scale).max().item()
    print(f"wide against drl_qnet_act f32 at {hidden}: {err:.3g}")
    assert err <= 2 * Q_TOL_EXACT, err


@gpu
@pytest.mark.parametrize("radius", [2, 3, 4])
def test_wide_code_input_equals_obs_input_bit_for_bit(radius):
    """A "code" net on drone 0's policy code gives the "obs" net's Q on the
    decoded windows bit for bit, and the same actions, at radius 2, 3 and 4."""
    obs, code = _windows(radius)
    n_in = obs.shape[1]
    a = _wide(n_in, (256, 128, 64), seed=radius)
    b = _wide(n_in, (256, 128, 64), seed=radius, inp="code")
    assert b.code_bytes == code.shape[1]
    for w0, w1 in zip((*a.weights, *a.biases), (*b.weights, *b.biases)):
        assert torch.equal(w0, w1)
    assert torch.equal(a.packed, b.packed)  # (one image: the code is decoded into the obs net's staging)
    for E in (1, 17, 65, E_MAX):
        qa, qb = torch.empty((E, 5), device="cuda"), torch.empty((E, 5), device="cuda")
        aa = a.act(obs[:E], 0.25, seed=3, step=E, q_out=qa)
        ab = b.act(code[:E].contiguous(), 0.25, seed=3, step=E, q_out=qb)
        assert torch.equal(qa.view(torch.int32), qb.view(torch.int32)) and torch.equal(aa, ab), E
    with pytest.raises(ValueError):
        b.act(obs, 0.0)
    a.check_errors()
    b.check_errors()


@gpu
@pytest.mark.parametrize("where", ["load", "input", "hidden", "nan", "packed_weight", "ok"])
def test_wide_range_is_checked_and_flagged(where):
    """tests/test_dqn.py's range checks on the wide path: a weight of 70000 is
    refused at load (and an infinite bias; a large finite bias is a valid
    net); an input, a hidden activation or a packed weight outside fp16's
    split range raises DRL_ERR_QNET_RANGE at check_errors."""
    from dronerl_amd._native import DroneRLError
    from dronerl_amd.dqn import _check, _stream, _vp
    x = _rows("window", 294)[:100].clone()
    net = _wide(294, (256, 64), seed=5)
    if where == "load":
        w = [t.clone() for t in net.weights]
        w[0][0, 0] = 70000.0
        with pytest.raises(ValueError, match="65504"):
            net.load(w, net.biases)
        b = [t.clone() for t in net.biases]
        b[0][3] = float("inf")
        with pytest.raises(ValueError, match="finite"):
            net.load(net.weights, b)
        b[0][3], b[1][2] = 1e6, -2e5
        net.load(net.weights, b)  # (the biases stay f32: a valid net, whose 1e6 activation an act would flag)
        return
    elif where == "input":
        x[17, 3] = 1.0e5
    elif where == "nan":
        x[42, 0] = float("nan")
    elif where == "hidden":  # weights in range, activations of layer 0 beyond it
        w = [t.clone() for t in net.weights]
        w[0][:, :] = 3000.0
        net.load(w, net.biases)
    elif where == "packed_weight":  # packed through the C ABI (no host check)
        w = [t.clone() for t in net.weights]
        w[2][1, 0] = 70000.0
        wp = (_vp * 3)(*[t.data_ptr() for t in w])
        bp = (_vp * 3)(*[t.data_ptr() for t in net.biases])
        _check(net.L, net.L.drl_widenet_pack(ctypes.byref(net.desc), wp, bp, _vp(net.packed.data_ptr()),
                                             _stream(net.device)))
        assert int(net.packed[-4].item()) != 0
    net.act(x, epsilon=0.0)
    if where == "ok":
        net.check_errors()
        return
    with pytest.raises(DroneRLError, match="fp16 split range"):
        net.check_errors()
    net.check_errors()  # cleared
    if where == "packed_weight":
        net.pack()  # a fresh pack of in-range weights clears the image's status
        assert int(net.packed[-4].item()) == 0
        net.act(x, epsilon=0.0)
        net.check_errors()


# ---- the learner (tests/test_large_batch_learner.py's loop and assertions) ----
def _net_and_target(sizes, inp, seed, cls=None):
    from dronerl_amd.dqn import WideQNetwork
    g = torch.Generator().manual_seed(seed + 5)
    if cls is None:
        net = WideQNetwork(sizes[0], sizes[1:-1], n_actions=sizes[-1], generator=g, input=inp)
    else:
        net = cls(sizes[0], sizes[1:-1], n_actions=sizes[-1], generator=g, precision="f32", input=inp)
    gb = torch.Generator(device="cuda").manual_seed(seed + 6)
    for b in net.biases:
        b.normal_(0, 0.05, generator=gb)
    net.pack()
    target = ([torch.randn(w.shape, generator=g) * 0.1 for w in net.weights],
              [torch.randn(b.shape, generator=g) * 0.05 for b in net.biases])
    return net, target


def _setup(sizes, inp, hp_kw, E, cap, seed=0, learner_cls=None, net_cls=None):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams, ReplayBuffer, WideDQNLearner
    radius = {150: 2, 294: 3}[sizes[0]]
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=radius), E)
    env.reset(seed=seed)
    net, target = _net_and_target(sizes, inp, seed, net_cls)
    hp = DQNHParams(**hp_kw)
    learner = (learner_cls or WideDQNLearner)(net, hp, target=target)
    rb = ReplayBuffer(cap, sizes[0], torch.device("cuda"), code_radius=radius if inp == "code" else 0)
    return env, net, learner, rb, hp


class _Loop:
    """train_jax.py's loop shape around a learner: the other drones' random
    actions, drone 0's act with the device epsilon, step, add_many (the caller
    trains)."""

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
        self.env.synth_actions(seed=5, step=self.t, out=self.acts)
        self.net.act(x, self.learner.epsilon, seed=3, step=self.t, actions=self.acts)
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
    """The act's packed image is the online net's: a fresh drl_widenet_pack of
    the same parameters is byte-identical."""
    after = net.packed.clone()
    net.pack()
    torch.cuda.synchronize()
    assert torch.equal(after, net.packed)


# net, input, hyperparameters, envs per step, ring capacity, steps, trained steps at least
ORACLE_CASES = [
    ((294, 256, 128, 64, 5), "code", dict(batch=8), 64, 300, 12, 12),
    # (the ring holds exactly one batch, and wraps)
    ((294, 136, 5), "obs", dict(batch=65, tau=0.6, target_update_interval=3), 50, 65, 12, 11),
    ((150, 256, 256, 256, 5), "obs", dict(batch=130), 64, 200, 12, 10),
    ((294, 200, 72, 5), "code", dict(batch=1000), 512, 4000, 8, 7),
]
ORACLE_IDS = ["sweep-net-b8", "136-obs-b65-ring-of-one-batch", "256x3-radius2-obs-b130", "200-72-b1000"]


@gpu
@pytest.mark.parametrize("sizes,inp,hp_kw,E,cap,steps,min_trained", ORACLE_CASES, ids=ORACLE_IDS)
def test_wide_learner_matches_oracle_bit_exact(sizes, inp, hp_kw, E, cap, steps, min_trained):
    """The train_jax.py loop shape with the wide act and learner on: act
    (device epsilon) -> step -> add_many -> drl_widenet_dqn_train.  Before
    each train the ring is copied to the host and the oracle takes the same
    step: all four parameter sets, the loss, every counter and both beta
    powers are equal bit for bit after every step; the trained-step count
    follows from E, batch and cap, so no case passes by never sampling; the
    image is byte-equal to a fresh drl_widenet_pack."""
    from dronerl_amd.dqn import WideDQNLearner, make_learner
    env, net, learner, rb, hp = _setup(sizes, inp, hp_kw, E, cap)
    assert isinstance(learner, WideDQNLearner) and type(make_learner(_net_and_target(sizes, inp, 1)[0], hp)) is WideDQNLearner
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
def test_wide_learner_equals_the_large_batch_learner_at_128_64():
    """A (128, 64) net: WideDQNLearner's parameter sets and counters equal
    LargeBatchDQNLearner's bit for bit over 12 steps from identical initial
    states on the same ring (the chain is the same; only the image differs)."""
    from dronerl_amd.dqn import LargeBatchDQNLearner, QNetwork, WideDQNLearner
    sizes, kw = (294, 128, 64, 5), dict(batch=96, tau=0.7, target_update_interval=3)
    env, net_a, a, rb, _ = _setup(sizes, "code", kw, 40, 300)
    _, net_b, b, _, _ = _setup(sizes, "code", kw, 40, 300, learner_cls=LargeBatchDQNLearner, net_cls=QNetwork)
    assert type(a) is WideDQNLearner and type(b) is LargeBatchDQNLearner
    assert bytes(a.layout) == bytes(b.layout)
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
    assert a.counters()["count"] == 10  # (40, 80 < 96 rows at the first two steps)
    a.check_errors()
    b.check_errors()
    _assert_packed_is_fresh(net_a)
    _assert_packed_is_fresh(net_b)


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
    return rb, nxt


@gpu
def test_wide_sample_slots_are_the_learners_draws():
    """WideDQNLearner.sample_slots (drl_widenet_dqn_sample_rows) == the
    oracle's sample_indices at the device step, step after step, for a batch
    of 300; refused for an empty ring."""
    from dronerl_amd.dqn import DQNHParams, WideDQNLearner
    from dronerl_amd.handle import DroneRLError
    rb, _ = _code_ring(900)
    net, target = _net_and_target((294, 136, 5), "code", seed=2)
    learner = WideDQNLearner(net, DQNHParams(batch=300, sample_seed=77), target=target)
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
def test_wide_act_and_train_are_graph_capturable():
    """One act + train (the sweep net, batch 257) captured with
    torch.cuda.graph and replayed 6 times equals 6 eager act + train calls on
    a twin bit for bit: the chain is linear (no parallel branches), the step,
    Adam's count and epsilon live on the device, and each replay's act reads
    the image the replay before it packed."""
    from dronerl_amd.dqn import DQNHParams, WideDQNLearner
    rb, code = _code_ring(900)
    hp = DQNHParams(batch=257, tau=0.6, target_update_interval=3, epsilon_decay_every=2)

    def make():
        net, target = _net_and_target((294, 256, 128, 64, 5), "code", seed=4)
        return net, WideDQNLearner(net, hp, target=target)

    (net_e, eager), (net_g, graphed) = make(), make()
    acts_e = torch.zeros((900, 1), dtype=torch.int32, device="cuda")
    acts_g, q_e, q_g = acts_e.clone(), torch.zeros((900, 5), device="cuda"), torch.zeros((900, 5), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            net_g.act(code, graphed.epsilon, seed=3, step=0, actions=acts_g, q_out=q_g)
            graphed.train(rb)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert graphed.counters()["step"] == 0  # (capturing runs nothing)
    for _ in range(6):
        g.replay()
        net_e.act(code, eager.epsilon, seed=3, step=0, actions=acts_e, q_out=q_e)
        eager.train(rb)
    torch.cuda.synchronize()
    assert eager.counters()["step"] == 6 and eager.counters()["count"] == 6
    for k in SETS:
        assert torch.equal(eager.sets[k].view(torch.int32), graphed.sets[k].view(torch.int32)), k
    assert eager.counters() == graphed.counters()
    assert torch.equal(net_e.packed, net_g.packed)
    assert torch.equal(q_e.view(torch.int32), q_g.view(torch.int32)) and torch.equal(acts_e, acts_g)
    _assert_packed_is_fresh(net_g)
    net_g.check_errors()


@gpu
def test_train_a_wide_net_end_to_end(tmp_path):
    """train(..., hidden=(256, 128, 64)) runs the loop on a WideQNetwork
    (input "code") with WideDQNLearner; the learner saves in the three
    checkpoint formats and to_qnet reloads each as a WideQNetwork whose Q is
    bit-identical to the live net's; evaluate works through the common act."""
    from dronerl_amd import EnvParams
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import WideDQNLearner, WideQNetwork
    from dronerl_amd.train import evaluate, train
    p = EnvParams(n_drones=4, grid_size=9)
    res = train(p, 512, 60, hidden=(256, 128, 64))
    assert isinstance(res.net, WideQNetwork) and res.net.input == "code" and isinstance(res.learner, WideDQNLearner)
    c = res.learner.counters()
    assert c["step"] == 60 and c["count"] == 60 and np.isfinite(c["loss"])
    code = res.env.get_code()
    q_live = torch.empty((512, 5), device="cuda")
    res.net.act(code, 0.0, q_out=q_live)
    obs = res.env.get_obs(1).reshape(512, -1)
    for fmt in ("torch", "jax", "torch_agent"):
        path = str(tmp_path / f"agent_{fmt}.safetensors")
        res.learner.save(path, format=fmt)
        ck = read_checkpoint(path)
        assert tuple(ck.dense_layers) == (256, 128, 64)
        back = to_qnet(ck, device="cuda")
        assert isinstance(back, WideQNetwork) and back.hidden == (256, 128, 64) and back.input == "obs"
        q_back = torch.empty((512, 5), device="cuda")
        back.act(obs, 0.0, q_out=q_back)
        assert torch.equal(q_back.view(torch.int32), q_live.view(torch.int32)), fmt
    agent, rnd, table = evaluate(p, back, num_evals=2, num_eval_steps=200, device="cuda")
    assert table.shape == (2, 2) and -1.0 <= agent[0] <= 1.0
    with pytest.raises(ValueError, match="wider than 128"):
        train(p, 512, 4, hidden=(256, 128, 64), world=2)


@gpu
def test_train_main_cli_with_the_sweep_net(tmp_path):
    """`python -m dronerl_amd.train --hidden_layers 256 128 64` just works:
    train, save both checkpoints, run the final eval, return the metrics."""
    from dronerl_amd.checkpoint import read_checkpoint
    from dronerl_amd.train import main
    m = main(["--num_envs", "512", "--num_steps", "60", "--hidden_layers", "256", "128", "64", "--num_evals", "2",
              "--num_eval_steps", "200", "--save_final_checkpoint", "--output_dir", str(tmp_path)])
    assert m["obs_per_sec"] > 0 and m["num_gpus"] == 1
    assert -1.0 <= m["eval_reward_mean"] <= 1.0 and -1.0 <= m["random_reward_mean"] <= 1.0
    assert tuple(read_checkpoint(m["checkpoint_torch"]).dense_layers) == (256, 128, 64)
