"""Convolutional Q-networks on the device (include/dronerl.h drl_convnet_*,
dronerl_amd.dqn.ConvQNetwork, checkpoint.to_qnet): Q and the greedy action
against host f32 and f64 forwards (torch.nn.functional.conv2d on the CPU), the
policy-code input bit for bit against the observation input, the reference's
own conv agent (sample_models/dqn-agent-5) on the recorded evaluator windows,
QNetwork.act's exploration stream, and the validation of every limit.

Tolerance: the project's criterion for the fp16 hi/lo split scheme
(tests/test_dqn.py Q_TOL_EXACT): |Q - ref| / (1 + max_a |ref|) <= 1e-5.
"""
import ctypes
import functools
import glob
import os
import re

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
Q_TOL_EXACT = 1e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _c(out_channels, kernel_size, stride, padding):
    return {"out_channels": out_channels, "kernel_size": kernel_size, "stride": stride, "padding": padding}


# case -> (W, conv layers, dense widths)
NETS = {
    "a": (7, (_c(4, 3, 1, 1),), (8,)),                       # the agent-5 shape: Cout below a tile
    "b": (7, (_c(8, 3, 1, 1),), ()),                         # train_jax default: flatten 392 into the Q head
    "c": (9, (_c(8, 3, 1, 0), _c(12, 3, 2, 1)), (16, 8)),    # two layers, stride 2, Cout 12, mixed padding
    "d": (5, (_c(5, 5, 1, 2),), (128,)),                     # odd channel count, K = 150, widest dense
    "e": (3, (_c(32, 1, 1, 0),), (8,)),                      # 1x1 kernel, widest Cout, smallest window
    "f": (7, (_c(6, 2, 3, 0),), ()),                         # even kernel, stride 3, floor of the map side
}
E_MAX = 300


def _params(W, conv, dense, n_actions=5, seed=0):
    """Seeded host parameters in torch layout: he-normal conv and hidden dense weights, lecun-normal head,
    biases ~ N(0, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    cw, cb, dw, db = [], [], [], []
    side, cin = W, 6
    for c in conv:
        k, co = c["kernel_size"], c["out_channels"]
        cw.append(torch.randn((co, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        cb.append(torch.randn(co, generator=g) * 0.1)
        side, cin = (side + 2 * c["padding"] - k) // c["stride"] + 1, co
    sizes = [side * side * cin, *dense, n_actions]
    for i in range(len(sizes) - 1):
        scale = 2.0 if i < len(sizes) - 2 else 1.0
        dw.append(torch.randn((sizes[i + 1], sizes[i]), generator=g) * (scale / sizes[i]) ** 0.5)
        db.append(torch.randn(sizes[i + 1], generator=g) * 0.1)
    return cw, cb, dw, db


def _host_q(params, conv, x, dtype):
    """torch ConvQNetwork.forward (dqn.py:153-159) on the CPU: x [E, W, W, 6]."""
    cw, cb, dw, db = params
    h = x.to(dtype).permute(0, 3, 1, 2)
    for c, w, b in zip(conv, cw, cb):
        h = torch.relu(torch.nn.functional.conv2d(h, w.to(dtype), b.to(dtype), stride=c["stride"],
                                                  padding=c["padding"]))
    h = h.flatten(1)
    for i, (w, b) in enumerate(zip(dw, db)):
        h = h @ w.to(dtype).t() + b.to(dtype)
        if i < len(dw) - 1:
            h = torch.relu(h)
    return h


@functools.lru_cache(maxsize=None)
def _windows(W):
    """Real env windows (the charge channel holds non-binary values): f32 [E_MAX, 3, W, W, 6] on the device."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=(W - 1) // 2), E_MAX)
    env.reset(seed=3)
    for t in range(5):
        env.step(env.synth_actions(seed=1, step=t))
    obs = env.get_obs(3)
    torch.cuda.synchronize()
    env.check_errors()
    return obs.reshape(E_MAX, 3, W, W, 6)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's net on the device, its host parameters and its two host references on E_MAX windows."""
    from dronerl_amd.dqn import ConvQNetwork
    W, conv, dense = NETS[name]
    params = _params(W, conv, dense, seed=sum(map(ord, name)))
    net = ConvQNetwork((W, W, 6), conv, dense)
    net.load(*params)
    x = _windows(W)[:, 1].cpu()
    assert float(x[..., 4].max()) > 0 and not torch.equal(x[..., 4], x[..., 4].round())  # non-binary charge
    return net, params, _host_q(params, conv, x, torch.float32), _host_q(params, conv, x, torch.float64)


@gpu
@pytest.mark.parametrize("E", [1, 17, 300])
@pytest.mark.parametrize("name", sorted(NETS))
def test_convnet_q_and_greedy_match_host_forward(name, E):
    _need_gpu()
    net, params, ref32, ref64 = _case(name)
    W, conv, dense = NETS[name]
    ref32, ref64 = ref32[:E], ref64[:E]
    obs = _windows(W)[:E, 1]          # a strided column of [E, 3, W, W, 6]: no copy
    assert not obs.is_contiguous() or E == 1
    q = torch.empty((E, 5), device="cuda")
    a = net.act(obs, 0.0, q_out=q)
    torch.cuda.synchronize()
    net.check_errors()
    qc = q.cpu()
    scale = 1 + ref32.abs().max(dim=1, keepdim=True).values
    err32 = ((qc - ref32).abs() / scale).max().item()
    err64 = ((qc.double() - ref64).abs() / scale.double()).max().item()
    print(f"case {name} E {E}: err vs f32 {err32:.3e}, vs f64 {err64:.3e}")
    assert err32 <= Q_TOL_EXACT, err32
    assert err64 <= Q_TOL_EXACT, err64
    act = a[:, 0].cpu().long()
    assert torch.equal(act, torch.argmax(qc, dim=1))       # the first argmax of its own Q
    if E > 1:
        top2 = torch.topk(ref32, 2, dim=1).values
        tol = 2 * Q_TOL_EXACT * scale[:, 0]
        clear = (top2[:, 0] - top2[:, 1]) > tol
        assert torch.equal(act[clear], torch.argmax(ref32, dim=1)[clear])
        chosen = ref32.gather(1, act[:, None])[:, 0]
        assert torch.all(chosen >= top2[:, 0] - tol)
    # reference_q (the class's plain torch forward) agrees with the host forward
    rq = net.reference_q(obs).cpu()
    assert ((rq - ref32).abs() / scale).max().item() <= Q_TOL_EXACT


@gpu
@pytest.mark.parametrize("W", [5, 7, 9])
def test_convnet_code_input_equals_obs_input(W):
    _need_gpu()
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import ConvQNetwork
    E = 300
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16, window_radius=(W - 1) // 2), E)
    env.reset(seed=5)
    code = env.new_code()
    for t in range(6):
        _, _, obs = env.step(env.synth_actions(seed=2, step=t), obs_k=1, code=code)
    conv, dense = (_c(8, 3, 1, 1), _c(5, 2, 2, 0)), (16,)
    params = _params(W, conv, dense, seed=W)
    nets = {}
    for inp in ("obs", "code"):
        nets[inp] = ConvQNetwork((W, W, 6), conv, dense, input=inp)
        nets[inp].load(*params)
    qo, qc = torch.empty((E, 5), device="cuda"), torch.empty((E, 5), device="cuda")
    ao = nets["obs"].act(obs.reshape(E, -1), 0.0, q_out=qo)
    ac = nets["code"].act(code, 0.0, q_out=qc)
    torch.cuda.synchronize()
    nets["obs"].check_errors()
    nets["code"].check_errors()
    assert float(qo.abs().max()) > 0
    assert torch.equal(qo, qc)
    assert torch.equal(ao, ac)


@functools.lru_cache(maxsize=None)
def _agent5_windows():
    """Episode 0 (seed 845) of each of the five submissions on the CPU oracle, driven by the recorded actions:
    the windows of agent index 5 (baseline-5), and for submission 5 also index 0, with the recorded actions."""
    from dronerl_amd.params import side_from_density
    from oracle.oracle import OracleEnv, Params
    rec = np.load(os.path.join(GOLD, "evaluator_scores.npz"))["actions0"]   # [submission, step, agent]
    p = Params(side=side_from_density(6, 0.05), n_drones=6)
    wins, acts = [], []
    for s in range(5):
        env = OracleEnv(p)
        env.seed(845)
        env.reset()
        for t in range(200):
            ob = np.asarray(env.obs(3, 6), dtype=np.float32).reshape(6, 7, 7, 6)
            for idx in ([5, 0] if s == 4 else [5]):
                wins.append(ob[idx].copy())
                acts.append(int(rec[s, t, idx]))
            env.step(rec[s, t].astype(np.int64))
    return np.stack(wins), np.array(acts)


@gpu
def test_convnet_reference_conv_agent_reproduces_recorded_actions(tmp_path):
    _need_gpu()
    from safetensors.numpy import save_file
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import ConvQNetwork
    path = os.path.join(GOLD, "sample_models", "dqn-agent-5.safetensors")
    ck = read_checkpoint(path)
    net = to_qnet(ck, device="cuda")
    assert isinstance(net, ConvQNetwork)
    wins, acts = _agent5_windows()
    assert wins.shape == (1200, 7, 7, 6)
    x = torch.from_numpy(wins).cuda()
    q = torch.empty((1200, 5), device="cuda")
    a = net.act(x, 0.0, q_out=q)       # one launch for the 1,200 windows
    torch.cuda.synchronize()
    net.check_errors()
    # a window may be excused only if its float64 top-two gap is below 2e-5 (1 + max|Q|): none is
    params = ([torch.from_numpy(np.array(ck.tensors["network.conv2d_1.weight"]))],
              [torch.from_numpy(np.array(ck.tensors["network.conv2d_1.bias"]))],
              [torch.from_numpy(np.array(ck.tensors[f"network.dense_{i}.weight"])) for i in (1, 2)],
              [torch.from_numpy(np.array(ck.tensors[f"network.dense_{i}.bias"])) for i in (1, 2)])
    ref64 = _host_q(params, ck.conv_layers, torch.from_numpy(wins), torch.float64)
    top2 = torch.topk(ref64, 2, dim=1).values
    gap = (top2[:, 0] - top2[:, 1]) / (1 + ref64.abs().max(dim=1).values)
    excused = gap < 2e-5
    print(f"smallest normalised gap {gap.min().item():.3e}; excused {int(excused.sum())}")
    assert int(excused.sum()) == 0
    got = a[:, 0].cpu().numpy()
    assert np.array_equal(got, acts), np.nonzero(got != acts)[0][:10]
    # a jax-format copy of the same checkpoint (Conv kernels [kh][kw][in][out], Dense kernels [in][out])
    jp = {}
    for k, v in ck.tensors.items():
        _, layer, what = k.split(".")
        name, idx = layer.split("_")
        jl = ("Dense" if name == "dense" else "Conv") + "_" + str(int(idx) - 1)
        if what == "weight":
            v = v.T if name == "dense" else np.transpose(v, (2, 3, 1, 0))
            what = "kernel"
        jp[f"params.{jl}.{what}"] = np.ascontiguousarray(v)
    md = {"network_type": "conv", "obs_shape": "(7, 7, 6)", "action_shape": "(5,)", "checkpoint_format": "jax",
          "conv_layers": str(ck.conv_layers), "conv_dense_layers": str(ck.dense_layers), "dense_layers": "(32, 32)"}
    jpath = str(tmp_path / "jax.safetensors")
    save_file(jp, jpath, metadata=md)
    qj = torch.empty((1200, 5), device="cuda")
    to_qnet(read_checkpoint(jpath), device="cuda").act(x, 0.0, q_out=qj)
    torch.cuda.synchronize()
    assert torch.equal(qj, q)


@gpu
def test_convnet_exploration_is_qnetworks_stream():
    _need_gpu()
    from dronerl_amd.dqn import ConvQNetwork, QNetwork
    E, W = 300, 7
    obs = _windows(W)[:, 1]
    g = torch.Generator().manual_seed(11)
    dense = QNetwork(W * W * 6, (32,), generator=g)
    net = ConvQNetwork((W, W, 6), NETS["a"][1], NETS["a"][2], generator=g)
    kw = dict(seed=1234567, step=9, env_offset=4000)
    rnd = net.act(obs, 1.0, **kw).clone()
    assert torch.equal(rnd, dense.act(obs, 1.0, **kw))           # epsilon 1: the random action column
    assert len(torch.unique(rnd)) == 5
    d_eps, d_greedy = dense.act(obs, 0.3, **kw).clone(), dense.act(obs, 0.0, **kw).clone()
    c_eps, c_greedy = net.act(obs, 0.3, **kw).clone(), net.act(obs, 0.0, **kw).clone()
    explored = (d_eps != d_greedy)[:, 0]
    assert 0.1 < explored.float().mean().item() < 0.4
    assert torch.equal(c_eps[explored], rnd[explored])            # the same envs explore, the same actions
    rest = ~explored
    assert torch.all((c_eps[rest] == c_greedy[rest]) | (c_eps[rest] == rnd[rest]))
    assert (c_eps != c_greedy).any()
    # env_offset shard invariance
    shard = net.act(obs[100:200], 0.3, seed=kw["seed"], step=kw["step"], env_offset=kw["env_offset"] + 100)
    assert torch.equal(shard, c_eps[100:200])
    # a one-element device epsilon
    eps = torch.tensor([0.3], device="cuda")
    assert torch.equal(net.act(obs, eps, **kw), c_eps)
    # one captured act with the device epsilon: a single kernel, no parallel branches
    out = torch.full((E, 1), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.act(obs, eps, actions=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.act(obs, eps, actions=out, **kw)
    out.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, c_eps)
    net.check_errors()
    # argument checks, as QNetwork.act's
    with pytest.raises(ValueError):
        net.act(obs.double(), 0.0)
    with pytest.raises(ValueError):
        net.act(obs, 0.0, actions=torch.empty((E + 1, 1), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        net.act(obs, 0.0, q_out=torch.empty((E, 4), device="cuda"))
    with pytest.raises(ValueError):
        net.act(obs, torch.zeros(2, device="cuda"))


# ------------------------------------------------------------- validation ---
def _packed_bytes(desc):
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind_convnet
    L = _bind_convnet(lib())
    nb = ctypes.c_int64()
    rc = L.drl_convnet_packed_bytes(ctypes.byref(desc), ctypes.byref(nb))
    return rc, L.drl_last_error().decode(), nb.value


@pytest.mark.parametrize("field,kw", [
    ("window", dict(W=4)), ("window", dict(W=11)), ("window", dict(W=1, conv=(_c(4, 1, 1, 0),))),
    ("out_channels", dict(conv=(_c(0, 3, 1, 1),))), ("out_channels", dict(conv=(_c(33, 3, 1, 1),))),
    ("kernel_size", dict(conv=(_c(4, 0, 1, 1),))), ("kernel_size", dict(conv=(_c(4, 6, 1, 1),))),
    ("stride", dict(conv=(_c(4, 3, 0, 1),))), ("stride", dict(conv=(_c(4, 3, 4, 1),))),
    ("padding", dict(conv=(_c(4, 3, 1, -1),))), ("padding", dict(conv=(_c(4, 3, 1, 5),))),
    ("map side", dict(W=3, conv=(_c(4, 5, 1, 0),))),
    ("dense widths", dict(dense=(12,))), ("dense widths", dict(dense=(136,))),
    ("n_actions", dict(n_actions=0)), ("n_actions", dict(n_actions=9)),
    ("input", dict(W=3, conv=(_c(4, 3, 1, 1),), input="code")),
])
def test_convnet_limits_are_refused_by_name(field, kw):
    """Every limit is refused when the description is validated (no GPU: drl_convnet_packed_bytes), with a
    message that names the field."""
    from dronerl_amd.dqn import ConvQNetwork, convnet_desc
    W = kw.get("W", 7)
    args = ((W, W, 6), kw.get("conv", (_c(4, 3, 1, 1),)), kw.get("dense", (8,)), kw.get("n_actions", 5))
    rc, msg, _ = _packed_bytes(convnet_desc(*args, input=kw.get("input", "obs")))
    assert rc != 0 and field in msg, msg
    with pytest.raises(ValueError, match=field):   # the class refuses before any device work
        ConvQNetwork(*args, input=kw.get("input", "obs"))


def test_convnet_layer_counts_and_null_calls_fail_cleanly():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import ConvQNetwork, DrlConvnetDesc, _bind_convnet, convnet_desc
    with pytest.raises(ValueError, match="n_conv"):
        ConvQNetwork((7, 7, 6), (), (8,))
    with pytest.raises(ValueError, match="n_conv"):
        ConvQNetwork((7, 7, 6), (_c(4, 3, 1, 1),) * 4, (8,))
    with pytest.raises(ValueError, match="n_dense"):
        ConvQNetwork((7, 7, 6), (_c(4, 3, 1, 1),), (8, 8, 8))
    with pytest.raises(ValueError, match="square"):
        ConvQNetwork((7, 7, 6), ({"out_channels": 4, "kernel_size": (3, 2)},), (8,))
    with pytest.raises(ValueError, match="obs_shape"):
        ConvQNetwork((7, 5, 6), (_c(4, 3, 1, 1),), (8,))
    d = DrlConvnetDesc()
    d.window, d.n_conv, d.n_actions = 7, 0, 5
    rc, msg, _ = _packed_bytes(d)
    assert rc != 0 and "n_conv" in msg
    d = convnet_desc((7, 7, 6), (_c(4, 3, 1, 1),), (8,))
    d.n_dense = 3
    rc, msg, _ = _packed_bytes(d)
    assert rc != 0 and "n_dense" in msg
    # the accepted shapes: the sample net, train_jax's default (no hidden dense layer), the corners
    for args in [((7, 7, 6), (_c(4, 3, 1, 1),), (8,)), ((7, 7, 6), (_c(8, 3, 1, 1),), ()),
                 ((9, 9, 6), (_c(32, 5, 3, 4), _c(32, 5, 1, 4), _c(1, 5, 2, 0)), (128, 128), 8),
                 ((3, 3, 6), ({"out_channels": 1, "kernel_size": 1},), (), 1)]:
        rc, msg, nb = _packed_bytes(convnet_desc(*args))
        assert rc == 0 and nb > 0 and nb % 16 == 0, msg
    # NULL pointers, num_envs == 0 and misaligned rows fail (or return) before any launch
    L = _bind_convnet(lib())
    vp = ctypes.c_void_p
    good = convnet_desc((7, 7, 6), (_c(4, 3, 1, 1),), (8,))
    assert L.drl_convnet_packed_bytes(None, None) != 0 and b"NULL" in L.drl_last_error()
    assert L.drl_convnet_packed_bytes(ctypes.byref(good), None) != 0 and b"NULL" in L.drl_last_error()
    one = (vp * 1)(vp(64))
    two = (vp * 2)(vp(64), vp(64))
    assert L.drl_convnet_pack(ctypes.byref(good), None, one, two, two, vp(64), None) != 0
    assert b"NULL" in L.drl_last_error()
    assert L.drl_convnet_pack(ctypes.byref(good), one, one, (vp * 2)(vp(64), None), two, vp(64), None) != 0
    assert b"NULL" in L.drl_last_error()
    assert L.drl_convnet_pack(ctypes.byref(good), one, one, two, two, vp(72), None) != 0
    assert b"16-byte" in L.drl_last_error()

    def act(packed=vp(64), inp=vp(64), n=4, stride=294, eps=None, actions=vp(64), astride=1, desc=good):
        return L.drl_convnet_act(ctypes.byref(desc), packed, inp, n, stride, 0.0, eps, 0, 0, 0, actions, astride,
                                 None, None, None)
    assert act(n=0) == 0
    assert act(n=-1) != 0 and b"num_envs" in L.drl_last_error()
    assert act(packed=None) != 0 and b"NULL" in L.drl_last_error()
    assert act(inp=None) != 0 and b"NULL" in L.drl_last_error()
    assert act(actions=None) != 0 and b"NULL" in L.drl_last_error()
    assert act(inp=vp(68)) != 0 and b"8-byte" in L.drl_last_error()
    assert act(stride=295) != 0 and b"8-byte" in L.drl_last_error()
    assert act(stride=292) != 0 and b"obs_stride" in L.drl_last_error()
    assert act(packed=vp(72)) != 0 and b"16-byte" in L.drl_last_error()
    assert act(eps=vp(66)) != 0 and b"d_epsilon" in L.drl_last_error()
    assert act(astride=0) != 0 and b"action_stride" in L.drl_last_error()
    code = convnet_desc((7, 7, 6), (_c(4, 3, 1, 1),), (8,), input="code")
    assert act(inp=vp(72), desc=code) != 0 and b"16-byte" in L.drl_last_error()


def test_to_qnet_refuses_conv_checkpoint_with_dense_width_12():
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    ck = read_checkpoint(os.path.join(GOLD, "sample_models", "dqn-agent-5.safetensors"))
    assert ck.network_type == "conv"
    ck.dense_layers = (12,)
    with pytest.raises(ValueError, match="12"):
        to_qnet(ck, device="cuda")


@gpu
def test_convnet_load_refuses_without_changing_and_range_is_flagged():
    _need_gpu()
    from dronerl_amd._native import DroneRLError
    from dronerl_amd.dqn import ConvQNetwork
    W, conv, dense = NETS["a"]
    net = ConvQNetwork((W, W, 6), conv, dense, generator=torch.Generator().manual_seed(2))
    obs = _windows(W)[:64, 1]
    q0, q1 = torch.empty((64, 5), device="cuda"), torch.empty((64, 5), device="cuda")
    net.act(obs, 0.0, q_out=q0)
    packed = net.packed.clone()
    good = _params(W, conv, dense, seed=1)
    with pytest.raises(ValueError, match="shape"):
        net.load([good[0][0][:, :, :2]], good[1], good[2], good[3])
    with pytest.raises(ValueError, match="layer count"):
        net.load(good[0], good[1], good[2][:1], good[3])
    big = [w.clone() for w in good[2]]
    big[0][0, 0] = 65504.0
    with pytest.raises(ValueError, match="65504"):
        net.load(good[0], good[1], big, good[3])
    bigc = [w.clone() for w in good[0]]
    bigc[0][0, 0, 0, 0] = -70000.0
    with pytest.raises(ValueError, match="65504"):
        net.load(bigc, good[1], good[2], good[3])
    assert torch.equal(net.packed, packed)
    net.act(obs, 0.0, q_out=q1)
    torch.cuda.synchronize()
    assert torch.equal(q0, q1)
    net.check_errors()
    # in-range weights that drive a conv activation past 65520: DRL_ERR_QNET_RANGE
    hot = [torch.full_like(w, 60000.0) for w in good[0]]
    net.load(hot, [torch.zeros_like(b) for b in good[1]], good[2], good[3])
    net.act(obs, 0.0)
    with pytest.raises(DroneRLError, match="range"):
        net.check_errors()
    net.load(*good)                     # and the net recovers
    net.act(obs, 0.0, q_out=q1)
    net.check_errors()
    ref = _host_q(good, conv, obs.cpu(), torch.float32)
    assert ((q1.cpu() - ref).abs() / (1 + ref.abs().max(dim=1, keepdim=True).values)).max().item() <= Q_TOL_EXACT


# Every __global__ kernel of dronerl_amd/csrc/convnet/*.hip and the -m gpu test that launches it
# (tests/test_abi.py::test_every_kernel_has_a_gpu_test's rule for the new directory).
KERNEL_TESTS = {
    "drl_convnet_pack_kernel": "test_convnet.py::test_convnet_load_refuses_without_changing_and_range_is_flagged",
    "drl_convnet_act_kernel": "test_convnet.py::test_convnet_q_and_greedy_match_host_forward",
}


def test_every_convnet_kernel_has_a_gpu_test():
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "convnet", "*.hip")):
        src = open(f).read()
        for m in re.finditer(r"__global__", src):
            k = re.search(r"\b(drl_[a-z0-9_]+_kernel)\s*\(", src[m.end():m.end() + 300])
            if k:
                found.add(k.group(1))
    assert found and found == set(KERNEL_TESTS), (sorted(found - set(KERNEL_TESTS)), sorted(set(KERNEL_TESTS) - found))
    for kern, ref in KERNEL_TESTS.items():
        fname, test = ref.split("::")
        text = open(os.path.join(REPO, "tests", fname)).read()
        m = re.search(rf"^((?:@.*\n)*)def {test}\(", text, re.M)
        assert m and "@gpu" in m.group(1), (kern, ref)
