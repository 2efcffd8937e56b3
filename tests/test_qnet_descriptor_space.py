"""The act kernels and the learner off the env's windows: the part of the
descriptor space (include/dronerl.h drl_qnet_desc / drl_convnet_desc) that the
other files never launch.

Every other GPU test of a Q-network feeds it observation windows of an env (a
handful of non-zero cells, five of six channels exactly 0 or 1, in_features =
W*W*6 = 2 mod 4, rows packed back to back) and a head of 5 actions.  Here:

1. dense seeded randn rows (every feature non-zero with a non-zero fp16 lo
   half) through the obs-input dense acts, at in_features 4..512 in both
   residues mod 4, one-slice nets, odd slice counts, both f32 layouts, narrow
   widths, 1..8 actions and E on both sides of every tile boundary;
2. rows inside a wider buffer whose every other float is NaN (obs_stride >
   in_features): Q and actions bit-equal to the packed rows';
3. rows rescaled by powers of two against inversely rescaled layer-0 weights
   (the same real Q): the range of the fp16 hi/lo split, fp16 subnormals
   included, pinned at the project's tolerance;
4. the epilogue of every act kernel at 1, 2, 4, 6 and 8 actions, exactly, with
   a sentinel behind Q (the row pitch) and a head whose argmax lies in 5..7;
5. the conv act on dense windows, and the two accepted corner nets that were
   validated but never launched;
6. the learner on a dense synthetic ring with 1..8 actions and layer-0 widths
   in both residues mod 4, bit for bit against oracle/dqn_learner.py.

Tolerances are the project's own (tests/test_dqn.py): Q_TOL_EXACT = 1e-5 on
|Q - ref| / (1 + max_a |ref|) for the f32 scheme, against an f32 and an f64
host forward; Q_TOL_BF16 / Q_TOL_F32 for the bf16 act.  A numpy model of the
split scheme (float16 hi / lo pieces, the three products accumulated in f64)
gives 2-4e-7 on section 1's shapes, <= 4e-7 on section 3's rescaled rows and
<= 1.2e-6 on its mixed-exponent rows, so 1e-5 is not a tight fit.  Each
test prints its figures (pytest -s).

The clear share (envs whose f32 reference's top two Q values are further
apart than 2 * Q_TOL_EXACT * scale) must be >= 0.99 in the f32 tests; it
depends on the seeded inputs and the host forward only, and is 1.0 for all
of them.  The bf16 act is checked at Q_TOL_BF16's margin (2 * 2e-2 * (1 +
|Q|), about 0.1 between the top two of Q values that spread by about 1),
which 0.99 of randn rows cannot clear: there the floor is the one of
test_qnet_greedy_matches_torch_reference, > 0.5 (0.87 to 1.0 for these
inputs), and every env's action, safe or not, must have a reference Q within
that margin of the maximum.

One departure in section 4: ConvQNetwork.act has no synth argument, so for
the two conv kernels columns 1.. of the actions are checked to stay untouched
instead of equal to drl_synth_actions'.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import dqn_learner as O
from tests.test_convnet import NETS as CONV_NETS
from tests.test_convnet import _c, _host_q, _params
from tests.test_dqn import Q_TOL_BF16, Q_TOL_EXACT, Q_TOL_F32, _hash_explore
from tests.test_dqn_learner import assert_same, oracle_hparams, state_from_learner
from tests.test_policy_code import Q_TOL, _epilogue_inputs, _f32_forward, _nets

gpu = pytest.mark.gpu
NAN = float("nan")


def _f64_forward(net, x):
    """tests/test_policy_code.py _f32_forward in f64 (test_qnet_f32_matches_fp32_forward's second reference)."""
    ref = x.cpu().double()
    for i, (w, b) in enumerate(zip(net.weights, net.biases)):
        ref = ref @ w.cpu().double().t() + b.cpu().double()
        if i < len(net.weights) - 1:
            ref = torch.relu(ref)
    return ref


def _errs(q, ref32, ref64):
    """Worst |Q - ref| / (1 + max_a |ref32|) against the two host forwards, and the row scales."""
    qc = q.cpu()
    scale = 1.0 + ref32.abs().amax(dim=1, keepdim=True)
    err32 = ((qc - ref32).abs() / scale).max().item()
    err64 = ((qc.double() - ref64).abs() / scale.double()).max().item()
    return err32, err64, scale


def _clear(ref32, scale):
    """Envs whose f32 reference's top two Q values are further apart than 2 Q_TOL_EXACT scale."""
    top2 = torch.topk(ref32, 2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > 2 * Q_TOL_EXACT * scale[:, 0]


def _assert_greedy(act, q, ref32, scale, A):
    """act: the first argmax of the kernel's own Q row; the f32 reference's argmax on every clear env, and the
    clear share >= 0.99 (1.0 on the host for the seeded inputs of this file)."""
    assert torch.equal(act, torch.argmax(q.cpu(), dim=1))
    if A == 1:
        assert int(act.abs().max()) == 0
        return 1.0
    clear = _clear(ref32, scale)
    share = clear.float().mean().item()
    assert share >= 0.99, share
    assert torch.equal(act[clear], torch.argmax(ref32, dim=1)[clear])
    # on the others the chosen action's reference Q is within the tolerance of the maximum
    # (test_qnet_f32_matches_fp32_forward's last clause)
    chosen = ref32.gather(1, act[:, None])[:, 0]
    assert torch.all(chosen >= ref32.amax(dim=1) - 2 * Q_TOL_EXACT * scale[:, 0])
    return share


# ------------------------------------------------- 1. dense random rows ---
# (in_features, hidden, n_actions, E values).  drl_qnet_packed_bytes accepts every shape at both precisions (no
# replacement was needed).  The last shape is not in the issue's list: at 512 -> 96 layer 0's hi + lo fragments
# (192 KB) do not fit the LDS, so it is the one that runs drl_qnet_act_f32_kernel's other layout (lo fragments
# from global memory); every listed shape takes the layer-0-in-LDS one.
DENSE_SHAPES = [
    (4, (8,), 1, (1, 17)),                      # the smallest net: one quad per row, one action
    (6, (16, 16), 2, (15, 17)),                 # one straddle quad and nothing else
    (30, (24, 40, 8), 3, (16, 17)),             # one slice padded to the ring of 2, widths 24 / 40 / 8
    (32, (32, 32), 4, (17, 33)),                # exactly one slice
    (34, (48, 16), 6, (17, 100)),               # one slice and a straddle quad in the second
    (64, (64,), 7, (1, 17)),                    # exactly the ring
    (100, (96, 32), 8, (15, 17)),               # in % 4 == 0, 4 slices
    (256, (128, 64), 8, (16, 17, 100)),         # 8 slices: a multiple of 32, 16-B aligned rows
    (294, (128, 64), 8, (17, 33, 100)),         # the benchmark net's input with the widest head
    (294, (128, 128, 128), 6, (17, 33)),        # layer 0 fills the LDS (160 KB)
    (480, (64, 32), 5, (15, 16, 17)),           # 15 slices padded to 16
    (512, (64,), 8, (1, 17, 100)),              # the maximum
    (512, (96, 32), 5, (17, 33)),               # f32: layer 0's lo fragments from global memory
]
E_MAX = 100
_DENSE_CASES = [(i, E) for i, s in enumerate(DENSE_SHAPES) for E in s[3]]
_DENSE_IDS = ["%d-%s-a%d-E%d" % (DENSE_SHAPES[i][0], "x".join(map(str, DENSE_SHAPES[i][1])), DENSE_SHAPES[i][2], E)
              for i, E in _DENSE_CASES]


@functools.lru_cache(maxsize=None)
def _dense_case(i, precision):
    """Shape i's net (the class's own weight init, biases N(0, 0.1)), E_MAX randn rows on the device and the f32
    and f64 host forwards of those rows; built once and only read."""
    from dronerl_amd.dqn import QNetwork
    inf, hidden, A, _ = DENSE_SHAPES[i]
    g = torch.Generator().manual_seed(1000 + i)
    net = QNetwork(inf, hidden, n_actions=A, generator=g, precision=precision)
    for b in net.biases:
        b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    net.pack()
    x = torch.randn((E_MAX, inf), generator=g)
    return net, x.cuda(), _f32_forward(net, x), _f64_forward(net, x)


def _one_action_checks(net, x):
    """n_actions == 1: epsilon 1 draws only action 0."""
    a = net.act(x, epsilon=1.0, seed=11, step=5)
    assert int(a.abs().max()) == 0


@gpu
@pytest.mark.parametrize("i,E", _DENSE_CASES, ids=_DENSE_IDS)
def test_f32_obs_act_on_dense_rows(i, E):
    """drl_qnet_act_f32_kernel, both layouts: Q within Q_TOL_EXACT of the f32 and the f64 host forward."""
    net, x, ref32, ref64 = _dense_case(i, "f32")
    A = DENSE_SHAPES[i][2]
    x, ref32, ref64 = x[:E], ref32[:E], ref64[:E]
    q = torch.empty((E, A), device="cuda")
    a = net.act(x, epsilon=0.0, q_out=q)
    net.check_errors()
    err32, err64, scale = _errs(q, ref32, ref64)
    print(f"f32 dense {_DENSE_IDS[_DENSE_CASES.index((i, E))]}: err vs f32 {err32:.3e}, vs f64 {err64:.3e}")
    assert err32 <= Q_TOL_EXACT, err32
    assert err64 <= Q_TOL_EXACT, err64
    share = _assert_greedy(a[:, 0].cpu().long(), q, ref32, scale, A)
    print(f"  clear share {share:.3f}")
    if A == 1:
        _one_action_checks(net, x)


@gpu
@pytest.mark.parametrize("i,E", _DENSE_CASES, ids=_DENSE_IDS)
def test_bf16_obs_act_on_dense_rows(i, E):
    """drl_qnet_act_kernel: test_qnet_greedy_matches_torch_reference's criterion (Q_TOL_BF16 against the forward
    with bf16-rounded operands, Q_TOL_F32 against the plain one; the reference's action wherever its margin is
    safe at Q_TOL_BF16)."""
    net, x, _, _ = _dense_case(i, "bf16")
    A = DENSE_SHAPES[i][2]
    x = x[:E]
    q = torch.empty((E, A), device="cuda")
    a = net.act(x, epsilon=0.0, q_out=q)
    net.check_errors()
    ref = net.reference_q(x, bf16_operands=True)
    ref32 = net.reference_q(x)
    e16 = ((q - ref).abs() / (1 + ref.abs())).max().item()
    e32 = ((q - ref32).abs() / (1 + ref32.abs())).max().item()
    print(f"bf16 dense {_DENSE_IDS[_DENSE_CASES.index((i, E))]}: vs bf16-operand forward {e16:.3e}, vs f32 {e32:.3e}")
    assert e16 <= Q_TOL_BF16, e16
    assert e32 <= Q_TOL_F32, e32
    assert torch.equal(a[:, 0].long(), torch.argmax(q, dim=1))
    if A == 1:
        assert int(a.abs().max()) == 0
        _one_action_checks(net, x)
    else:
        top2 = torch.topk(ref, 2, dim=1).values
        margin = 2 * Q_TOL_BF16 * (1 + top2[:, 0].abs())
        safe = (top2[:, 0] - top2[:, 1]) > margin
        share = safe.float().mean().item()
        print(f"  safe share {share:.3f}")
        assert share > 0.5, share   # (the mirrored test's floor; E = 1: the one env is safe)
        assert torch.equal(a[safe, 0].long(), torch.argmax(ref, dim=1)[safe])
        chosen = ref.gather(1, a[:, :1].long())[:, 0]
        assert torch.all(chosen >= top2[:, 0] - margin)


# ------------------------------------- 2. rows inside a poisoned buffer ---
_SHAPE_OF_IN = {294: 8, 64: 5, 6: 1}  # in_features -> its DENSE_SHAPES entry (straddle, no straddle, one quad)


def _poisoned_view(rows, pad, lead=0):
    """`rows` [E, n] as a view of a buffer of NaNs with `pad` more floats per row (and `lead` in front)."""
    E, n = rows.shape
    buf = torch.full((lead + E * (n + pad),), NAN, device=rows.device)
    view = buf[lead:].view(E, n + pad)[:, :n]
    view.copy_(rows)
    assert view.stride(0) == n + pad and not bool(torch.isnan(view).any())
    return buf, view


@gpu
@pytest.mark.parametrize("pad,lead", [(2, 0), (10, 0), (38, 0), (10, 2)])
@pytest.mark.parametrize("inf", [294, 64, 6])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_dense_act_reads_only_its_rows(precision, inf, pad, lead):
    """obs_stride = in_features + pad: pad slots, clamped quads and the last env's tail stay inside [row, row +
    in_features), so no NaN reaches Q or the range flag.  Rows stay 8-byte aligned; at 64 features they fall
    alternately on and off 16-byte alignment, and lead = 2 moves every 294- and 6-feature row off it."""
    E = 17
    net, x, _, _ = _dense_case(_SHAPE_OF_IN[inf], precision)
    rows = x[:E]
    _, view = _poisoned_view(rows, pad, lead)
    A = net.n_actions
    q0, q1 = torch.empty((E, A), device="cuda"), torch.empty((E, A), device="cuda")
    a0 = net.act(rows, epsilon=0.25, seed=3, step=1, q_out=q0).clone()
    net.check_errors()
    a1 = net.act(view, epsilon=0.25, seed=3, step=1, q_out=q1)
    net.check_errors()
    assert bool(torch.isfinite(q0).all()) and float(q0.abs().max()) > 0
    assert torch.equal(q0, q1)
    assert torch.equal(a0, a1)


@gpu
@pytest.mark.parametrize("pad,lead", [(2, 0), (10, 0), (38, 0), (10, 2)])
@pytest.mark.parametrize("name", ["a", "e"])
def test_conv_act_reads_only_its_rows(name, pad, lead):
    """The conv obs act's staging on the same buffers (7x7 and 3x3 windows)."""
    E = 17
    net, _, x, _, _ = _conv_case(name)
    rows = x[:E].reshape(E, -1)
    _, view = _poisoned_view(rows, pad, lead)
    A = net.n_actions
    q0, q1 = torch.empty((E, A), device="cuda"), torch.empty((E, A), device="cuda")
    a0 = net.act(rows, 0.25, seed=3, step=1, q_out=q0).clone()
    net.check_errors()
    a1 = net.act(view, 0.25, seed=3, step=1, q_out=q1)
    net.check_errors()
    assert bool(torch.isfinite(q0).all()) and float(q0.abs().max()) > 0
    assert torch.equal(q0, q1)
    assert torch.equal(a0, a1)


# ------------------------------------------- 3. power-of-two rescaling ---
SCALE_NETS = [(294, (128, 64), 5), (512, (64,), 8), (6, (8,), 2)]
SCALE_E = 64


@functools.lru_cache(maxsize=None)
def _scale_case(j):
    """The net at s = 1, its rows, the mixed-exponent rows, and the f32 / f64 host forwards of both."""
    from dronerl_amd.dqn import QNetwork
    inf, hidden, A = SCALE_NETS[j]
    g = torch.Generator().manual_seed(3000 + j)
    net = QNetwork(inf, hidden, n_actions=A, generator=g, precision="f32")
    for b in net.biases:
        b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    net.pack()
    x = torch.randn((SCALE_E, inf), generator=g)
    k = torch.randint(-18, 4, (SCALE_E, inf), generator=g)          # uniform in [-18, 3]
    xm = torch.randn((SCALE_E, inf), generator=g) * torch.pow(2.0, k.float())
    refs = {"dense": (_f32_forward(net, x), _f64_forward(net, x)),
            "mixed": (_f32_forward(net, xm), _f64_forward(net, xm))}
    return net, x, xm, refs


@gpu
@pytest.mark.parametrize("s", ["2^-14", "1", "2^10", "mixed"])
@pytest.mark.parametrize("j", range(len(SCALE_NETS)), ids=["294-128x64-a5", "512-64-a8", "6-8-a2"])
def test_f32_split_range_under_power_of_two_rescaling(j, s):
    """Rows x * s against layer-0 weights W0 / s, s a power of two: both are exact in f32, so the real Q and both
    host forwards are those of s = 1, and only the fp16 pieces of the split move -- at s = 2^-14 almost every
    fp16(x) is subnormal, at s = 2^10 many fp16(W0 / s) are.  "mixed": randn * 2^k rows, k uniform in [-18, 3]
    per element, against the unscaled net.  Q stays within Q_TOL_EXACT of the f64 forward: v_cvt_f16_f32 and
    v_mfma_f32_16x16x32_f16 keep fp16 subnormals (include/dronerl.h DRL_QNET_F32's 2^-23 |v| claim)."""
    from dronerl_amd.dqn import QNetwork
    net, x, xm, refs = _scale_case(j)
    inf, hidden, A = SCALE_NETS[j]
    if s == "mixed":
        run, rows, (ref32, ref64) = net, xm, refs["mixed"]
    else:
        sv = {"2^-14": 2.0 ** -14, "1": 1.0, "2^10": 2.0 ** 10}[s]
        rows, (ref32, ref64) = x * sv, refs["dense"]
        w0 = net.weights[0].cpu() / sv
        assert torch.equal(w0 * sv, net.weights[0].cpu()) and torch.equal(rows / sv, x)   # exact rescaling
        run = QNetwork(inf, hidden, n_actions=A, precision="f32")
        run.load([w0, *net.weights[1:]], net.biases)
    q = torch.empty((SCALE_E, A), device="cuda")
    a = run.act(rows.cuda(), epsilon=0.0, q_out=q)
    run.check_errors()
    err32, err64, scale = _errs(q, ref32, ref64)
    print(f"rescaled {SCALE_NETS[j]} s = {s}: err vs f32 {err32:.3e}, vs f64 {err64:.3e}")
    assert err64 <= Q_TOL_EXACT, err64
    assert err32 <= Q_TOL_EXACT, err32
    _assert_greedy(a[:, 0].cpu().long(), q, ref32, scale, A)


# ------------------------------------- 4. every epilogue at 1..8 actions ---
SENTINEL = -12345.0
EPI_KERNELS = ["bf16_obs", "f32_obs", "code_32_32", "code4", "code2", "conv_obs", "conv_code"]
HEADS = [1, 2, 4, 6, 8, "8hot"]  # "8hot": 8 actions, the last three biases + 10 (the argmax lies in 5..7)


@functools.lru_cache(maxsize=None)
def _head_nets(hidden, head):
    """(code net, obs net, bf16 obs net) of the same parameters with an A-action head: the hidden layers are
    tests/test_policy_code.py _nets' (a pair with 5 actions), the head lecun-normal with N(0, 0.1) biases."""
    from dronerl_amd.dqn import QNetwork, flax_kernel_init
    A = 8 if head == "8hot" else head
    five, _ = _nets(294, hidden, seed=77)
    g = torch.Generator().manual_seed(4000 + A)
    hw = flax_kernel_init((A, hidden[-1]), 1.0, g)
    hb = torch.randn(A, generator=g) * 0.1
    if head == "8hot":
        hb[-3:] += 10.0
    ws, bs = [*five.weights[:-1], hw], [*five.biases[:-1], hb]
    nets = []
    for precision, inp in (("f32", "code"), ("f32", "obs"), ("bf16", "obs")):
        net = QNetwork(294, hidden, n_actions=A, precision=precision, input=inp)
        net.load(ws, bs)
        nets.append(net)
    return tuple(nets)


@functools.lru_cache(maxsize=None)
def _conv_head_nets(head):
    """(obs net, code net, host parameters) of test_convnet.NETS' case "a" with an A-action head."""
    from dronerl_amd.dqn import ConvQNetwork
    A = 8 if head == "8hot" else head
    W, conv, dense = CONV_NETS["a"]
    params = _params(W, conv, dense, n_actions=A, seed=4100 + A)
    if head == "8hot":
        params[3][-1][-3:] += 10.0
    nets = []
    for inp in ("obs", "code"):
        net = ConvQNetwork((W, W, 6), conv, dense, n_actions=A, input=inp)
        net.load(*params)
        nets.append(net)
    return nets[0], nets[1], params


def _q_buffer(E, A):
    """q_out [E, A] with sentinel floats behind it: 64, and E * (8 - A) more, so that a store at row pitch 8 or 5
    instead of A lands on sentinels inside the buffer."""
    buf = torch.full((E * 8 + 64,), SENTINEL, device="cuda")
    return buf, buf[:E * A].view(E, A)


def _assert_epilogue(acts, buf, q, A, eps, seed, step, off, synth):
    """Column 0: the exploration stream's draw (in [0, A)) where the env explores, the first argmax of the
    kernel's own Q row elsewhere; columns 1..: drl_synth_actions' (synth) or untouched; the floats behind Q
    untouched, Q itself written and finite."""
    from dronerl_amd import _native
    E, N = acts.shape
    assert bool((buf[E * A:] == SENTINEL).all())
    assert bool(torch.isfinite(q).all()) and not bool((q == SENTINEL).any())
    a, greedy = acts.cpu().numpy(), torch.argmax(q, dim=1).cpu().numpy()
    n_exp = 0
    for e in range(E):
        explores, rnd = _hash_explore(seed, step, off + e, A, eps)
        assert 0 <= rnd < A
        n_exp += explores
        assert a[e, 0] == (rnd if explores else greedy[e]), e
    assert 0 < n_exp < E
    if synth is None:
        assert (a[:, 1:] == -1).all()
    else:
        ref = torch.empty((E, N), dtype=torch.int32, device="cuda")
        assert _native.lib().drl_synth_actions(synth[0], synth[1], off, E, N, ref.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream) == 0
        assert np.array_equal(a[:, 1:], ref.cpu().numpy()[:, 1:])
    return greedy


@gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("kernel", EPI_KERNELS)
def test_every_act_epilogue_at_every_head(kernel, head, monkeypatch):
    """test_dense_act_epilogue_streams' check (the kernels selected as there, plus the conv act on both inputs)
    at 1, 2, 4, 6 and 8 actions: actions 4..7 come from the g = 1 lanes' registers (tile_act, the f32 act's own
    gather), the code2 / code4 kernels keep a rolled Q store, the conv act zero-fills q[n_actions..8).  The Q
    values: the f32 kernels' within Q_TOL_EXACT of the f32 host forward, a code net's within 2 Q_TOL of its obs
    net's, the conv pair's bit-equal.  "8hot": every env's argmax lies in 5..7.  The conv act takes no synth
    argument: its columns 1.. must stay untouched."""
    E, N = 31, 3
    eps, seed, step, off, synth = 0.3, 7, 3, 5000, (2024, 9)
    A = 8 if head == "8hot" else head
    code, x = _epilogue_inputs(E)
    if kernel == "code2":
        monkeypatch.setenv("DRL_QN_CODE", "2")
    acts = torch.full((E, N), -1, dtype=torch.int32, device="cuda")
    buf, q = _q_buffer(E, A)
    kw = dict(seed=seed, step=step, env_offset=off)
    if kernel.startswith("conv"):
        onet, cnet, params = _conv_head_nets(head)
        net, inp, other, oinp = (onet, x, cnet, code) if kernel == "conv_obs" else (cnet, code, onet, x)
        net.act(inp, eps, actions=acts, q_out=q, **kw)
        net.check_errors()
        greedy = _assert_epilogue(acts, buf, q, A, eps, seed, step, off, None)
        obuf, oq = _q_buffer(E, A)
        oacts = other.act(oinp, eps, q_out=oq, **kw)
        other.check_errors()
        assert torch.equal(q, oq) and bool((obuf[E * A:] == SENTINEL).all())
        assert torch.equal(oacts[:, 0], acts[:, 0])
        ref = _host_q(params, CONV_NETS["a"][1], x.reshape(E, 7, 7, 6).cpu(), torch.float32)
    else:
        hidden = (32, 32) if kernel == "code_32_32" else (128, 64)
        cnet, onet, bnet = _head_nets(hidden, head)
        net, inp = {"bf16_obs": (bnet, x), "f32_obs": (onet, x)}.get(kernel, (cnet, code))
        net.act(inp, epsilon=eps, actions=acts, q_out=q, synth=synth, **kw)
        net.check_errors()
        greedy = _assert_epilogue(acts, buf, q, A, eps, seed, step, off, synth)
        ref = _f32_forward(onet, x)
        if net is cnet:   # the code net's Q against its obs net's
            obuf, oq = _q_buffer(E, A)
            onet.act(x, epsilon=eps, q_out=oq, **kw)
            onet.check_errors()
            assert bool((obuf[E * A:] == SENTINEL).all())
            scale = 1.0 + ref.abs().amax(dim=1, keepdim=True)
            assert ((q.cpu() - oq.cpu()).abs() / scale).max().item() <= 2 * Q_TOL
            assert ((oq.cpu() - ref).abs() / scale).max().item() <= Q_TOL_EXACT
    scale = 1.0 + ref.abs().amax(dim=1, keepdim=True)
    if kernel == "bf16_obs":
        refb = net.reference_q(x, bf16_operands=True)
        assert bool(torch.all((q - refb).abs() <= Q_TOL_BF16 * (1 + refb.abs())))
    else:
        err = ((q.cpu() - ref).abs() / scale).max().item()
        print(f"epilogue {kernel} head {head}: err vs f32 {err:.3e}")
        assert err <= Q_TOL_EXACT, err
        if A > 1:
            clear = _clear(ref, scale)
            assert torch.equal(torch.from_numpy(greedy)[clear], torch.argmax(ref, dim=1)[clear])
    if head == "8hot":
        assert int(torch.argmax(ref, dim=1).min()) >= 5
        assert greedy.min() >= 5
    if A == 1:
        assert (acts[:, 0] == 0).all()


# -------------------------------------------- 5. conv nets, dense windows ---
# case -> (W, conv layers, dense widths, n_actions): test_convnet.NETS and the two corners that
# test_convnet_layer_counts_and_null_calls_fail_cleanly validates but nothing launches
CONV_CASES = {k: (*v, 5) for k, v in CONV_NETS.items()}
CONV_CASES["corner3"] = (9, (_c(32, 5, 3, 4), _c(32, 5, 1, 4), _c(1, 5, 2, 0)), (128, 128), 8)
CONV_CASES["corner1"] = (3, (_c(1, 1, 1, 0),), (), 1)
CONV_E_MAX = 33


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    """The case's net, its host parameters, CONV_E_MAX randn windows on the device and their two host forwards."""
    from dronerl_amd.dqn import ConvQNetwork
    W, conv, dense, A = CONV_CASES[name]
    params = _params(W, conv, dense, n_actions=A, seed=5000 + sum(map(ord, name)))
    net = ConvQNetwork((W, W, 6), conv, dense, n_actions=A)
    net.load(*params)
    x = torch.randn((CONV_E_MAX, W, W, 6), generator=torch.Generator().manual_seed(5100 + W))
    return net, params, x.cuda(), _host_q(params, conv, x, torch.float32), _host_q(params, conv, x, torch.float64)


@gpu
@pytest.mark.parametrize("E", [1, 17, 33])
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_act_on_dense_windows(name, E):
    """drl_convnet_act_kernel on randn windows: every tap x channel x position carries weight."""
    net, params, x, ref32, ref64 = _conv_case(name)
    A = CONV_CASES[name][3]
    ref32, ref64 = ref32[:E], ref64[:E]
    q = torch.empty((E, A), device="cuda")
    a = net.act(x[:E], 0.0, q_out=q)
    net.check_errors()
    err32, err64, scale = _errs(q, ref32, ref64)
    print(f"conv dense {name} E {E}: err vs f32 {err32:.3e}, vs f64 {err64:.3e}")
    assert err32 <= Q_TOL_EXACT, err32
    assert err64 <= Q_TOL_EXACT, err64
    act = a[:, 0].cpu().long()
    assert torch.equal(act, torch.argmax(q.cpu(), dim=1))
    if A > 1:
        clear = _clear(ref32, scale)
        assert torch.equal(act[clear], torch.argmax(ref32, dim=1)[clear])
    else:
        assert int(act.abs().max()) == 0
        assert int(net.act(x[:E], 1.0, seed=11, step=5).abs().max()) == 0


# ------------------------------------ 6. the learner on a dense ring ---
# (sizes, hyperparameters); drl_dqn_layout_query accepts every shape (no replacement was needed)
LEARNER_CASES = [
    ((64, 32, 3), dict(batch=8)),
    ((100, 48, 16, 8), dict(batch=16, tau=0.5, target_update_interval=2)),
    ((30, 8, 2), dict(batch=4)),
    ((294, 128, 64, 1), dict(batch=8)),
    ((256, 128, 128, 6), dict(batch=32)),
]
RING_CAP, RING_FILL, LEARNER_STEPS = 200, 150, 12


@gpu
@pytest.mark.parametrize("sizes,hp_kw", LEARNER_CASES, ids=["-".join(map(str, s)) for s, _ in LEARNER_CASES])
def test_learner_on_dense_ring_matches_oracle_bit_exact(sizes, hp_kw):
    """drl_dqn_train on a ring of dense randn rows (every layer-0 gradient non-zero), rewards N(0, 1), dones at
    p = 0.2 and actions uniform in [0, A) -- plus one row with action A and one with -1, which oracle and kernel
    define as contributing nothing, placed on slots the steps draw.  After each of 12 steps the parameters,
    target, moments, loss and counters equal oracle/dqn_learner.py's bit for bit; at the end the act's packed
    image is byte-equal to a fresh pack of the online parameters."""
    from dronerl_amd.dqn import DQNHParams, DQNLearner, QNetwork, ReplayBuffer
    n_in, A = sizes[0], sizes[-1]
    g = torch.Generator().manual_seed(6000 + n_in)
    net = QNetwork(n_in, sizes[1:-1], n_actions=A, generator=g, precision="f32")
    for b in net.biases:
        b.copy_(torch.randn(b.shape, generator=g) * 0.05)
    net.pack()
    hp = DQNHParams(**hp_kw)
    target = ([torch.randn(w.shape, generator=g) * 0.1 for w in net.weights],
              [torch.randn(b.shape, generator=g) * 0.05 for b in net.biases])
    learner = DQNLearner(net, hp, target=target)
    rb = ReplayBuffer(RING_CAP, n_in, torch.device("cuda"))
    n = RING_FILL
    obs, nobs = torch.randn((n, n_in), generator=g), torch.randn((n, n_in), generator=g)
    acts = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
    # the two out-of-range actions on slots that steps 1 and 2 sample
    s1 = O.sample_indices(hp.sample_seed, 1, hp.batch, n)[0]
    s2 = [s for s in O.sample_indices(hp.sample_seed, 2, hp.batch, n) if s != s1][-1]
    acts[s1], acts[s2] = A, -1
    rews = torch.randn(n, generator=g)
    dones = (torch.rand(n, generator=g) < 0.2).to(torch.uint8)
    rb.add_many(obs.cuda(), acts.cuda(), rews.cuda(), nobs.cuda(), dones.cuda())
    assert rb.size == n and rb.cursor == n
    ring = {k: getattr(rb, k).cpu().numpy().copy() for k in ("obs", "next_obs", "actions", "rewards", "dones")}
    assert np.array_equal(ring["obs"][:n], obs.numpy()) and np.array_equal(ring["next_obs"][:n], nobs.numpy())
    assert np.array_equal(ring["actions"][:n], acts.numpy()) and np.array_equal(ring["dones"][:n], dones.numpy())
    st, ohp = state_from_learner(learner), oracle_hparams(hp)
    seen = set()
    for t in range(LEARNER_STEPS):
        info = O.learner_step(st, ohp, ring["obs"], ring["next_obs"], ring["actions"], ring["rewards"],
                              ring["dones"], rb.size)
        assert info["trained"]
        seen.update(int(ring["actions"][s]) for s in info["rows"])
        learner.train(rb)
        torch.cuda.synchronize()
        assert_same(learner, st, t)
    learner.check_errors()
    net.check_errors()
    assert {A, -1} <= seen
    assert float(learner.counters()["loss"]) > 0
    after = net.packed.clone()
    net.pack()
    assert torch.equal(after, net.packed)
