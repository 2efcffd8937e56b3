"""Every launch whose kernel or addressing depends on a 32-bit bound of the buffer it is given, run at that bound
from both sides.

The other GPU tests run hundreds or thousands of rows; the branches pinned here exist only at millions of rows, so
these are the smallest shapes at which they run at all.  No big buffer has a host reference.  Its rows come from a
small pool of P_POOL rows (a prime: neither a power of two nor a multiple of a 16-row tile), big[e] = pool[h(e)]
with h(e) = (e * 2654435761 mod 2^32) mod P_POOL, so an offset that wraps, truncates or slips by a tile lands on
another pool row.  Every act kernel's Q row depends on its own input row alone, so the big launch must equal the
pool launch of the same kernel, out_big[e] == out_pool[h(e)], bit for bit on every row (compared on the device,
no sampling), and the pool launch is checked against the host f32 and f64 forwards at the project's tolerances
(tests/test_dqn.py Q_TOL_EXACT, Q_TOL_BF16, Q_TOL_F32).  The replay ring is checked against torch indexing, get_obs
and the synthetic actions against the CPU oracle.

Which kernel a launch takes is read off the launch code's own condition (launch_replay_add, launch_qnet_act_code,
launch_synth, qnet_act_impl); each test derives its bound from that condition and asserts the arithmetic.

The last test (no GPU) keeps a manifest of every size bound in dronerl_amd/csrc: a new or edited bound fails it
until the bound is listed with the test that runs it, or the reason it needs none.
"""
import functools
import glob
import os
import re

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_POOL = 4099               # pool rows (prime)
H_MULT = 2654435761         # Knuth's multiplicative hash constant
CHUNK = 1 << 22             # rows per device comparison (bounds the gathered expectation's size)


@pytest.fixture(autouse=True)
def _device_memory(request):
    """Each GPU test starts from an empty cache, gives its blocks back and prints its peak device memory."""
    on = request.node.get_closest_marker("gpu") is not None and torch.cuda.is_available()
    if on:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    yield
    if on:
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        torch.cuda.empty_cache()
        print(f"\n[peak device memory] {request.node.name}: {peak / 2**30:.2f} GiB")


def _pool_index(E, start=0, step=1):
    """h(e) of rows start, start + step, .. (E of them), int64 on the device."""
    e = torch.arange(E, dtype=torch.int64, device="cuda") * step + start
    return ((e * H_MULT) & 0xFFFFFFFF) % P_POOL


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_rows_from_pool(out_big, out_pool, idx, what):
    """out_big[e] == out_pool[idx[e]] for every row e, bit for bit, on the device.  A Q table must tell the pool
    rows apart (more than half of them distinct), or a slipped offset could pass."""
    assert out_big.shape[0] == idx.shape[0] and out_pool.shape[0] == P_POOL
    if out_pool.dtype == torch.float32:
        distinct = torch.unique(_bits(out_pool), dim=0).shape[0]
        assert distinct > P_POOL // 2, (what, distinct)
    b, p = _bits(out_big), _bits(out_pool)
    for s in range(0, b.shape[0], CHUNK):
        got, exp = b[s:s + CHUNK], p.index_select(0, idx[s:s + CHUNK])
        if not torch.equal(got, exp):
            bad = (got != exp).reshape(got.shape[0], -1).any(1).nonzero()[:8, 0] + s
            raise AssertionError(f"{what}: rows {bad.tolist()} differ from their pool rows "
                                 f"(of {int((got != exp).reshape(got.shape[0], -1).any(1).sum())} in this chunk)")


def _assert_exact_pool_q(net, q, act, x, what):
    """The pool launch of an f32 (fp16 hi/lo split) kernel against the host f32 and f64 forwards, as
    tests/test_qnet_descriptor_space.py does it: Q_TOL_EXACT, and the reference's greedy action."""
    from tests.test_dqn import Q_TOL_EXACT
    from tests.test_policy_code import _f32_forward
    from tests.test_qnet_descriptor_space import _assert_greedy, _errs, _f64_forward
    ref32, ref64 = _f32_forward(net, x), _f64_forward(net, x)
    err32, err64, scale = _errs(q, ref32, ref64)
    print(f"{what}: pool err vs f32 {err32:.3e}, vs f64 {err64:.3e}")
    assert err32 <= Q_TOL_EXACT, err32
    assert err64 <= Q_TOL_EXACT, err64
    _assert_greedy(act[:, 0].cpu().long(), q, ref32, scale, q.shape[1])


# ================================================================ 1. replay add: three kernels, two sides each ==
# launch_replay_add (dronerl_qnet.hip), rows = n - first landing rows of obs_floats floats, D4 = obs_floats / 4,
# D2 = obs_floats / 2:
#   drl_replay_add16_kernel   if the rows are 16-B vectors at 16-B aligned addresses and rows * D4 * D4 < 2^32
#   drl_replay_add_kernel     else if rows * D2 * D2 < 2^32
#   drl_replay_add_rows_kernel otherwise
# (obs_floats, the fast kernel's divisor of obs_floats, pad floats per batch row, batch larger than the ring, the
#  last row count the fast kernel takes, worked out by hand from the condition: at 2050 floats D2 = 1025 and
#  4088 * 1025^2 = 4,294,955,000 < 2^32 <= 4089 * 1025^2)
REPLAY_CASES = {
    "294-add": (294, 2, 0, False, 198758),      # the project's row: drl_replay_add_kernel | rows kernel
    "2050-add": (2050, 2, 4, True, 4088),       # = 2 mod 4, padded rows, n > capacity (first > 0)
    "4096-add16": (4096, 4, 4, False, 4095),    # 16-B rows (padded by one 16-B vector): drl_replay_add16_kernel
}
STALE = 0x5A5A5A5A


def _replay_run(D, cap, c0, n, obs, nobs, acts, rews, dones):
    """A stale ring of `cap` rows with its cursor at c0 after add_many of the batch's first n rows."""
    from dronerl_amd.dqn import ReplayBuffer
    rb = ReplayBuffer(cap, D, torch.device("cuda"))
    rb.obs.view(torch.int32).fill_(STALE)
    rb.next_obs.view(torch.int32).fill_(STALE)
    rb.actions.fill_(-7)
    rb.rewards.fill_(-7.0)
    rb.dones.fill_(77)
    rb.cursor = c0
    rb.add_many(obs[:n], acts[:n], rews[:n], nobs[:n], dones[:n])
    torch.cuda.synchronize()
    return rb


def _landing(cap, c0, n):
    """(batch rows that land, their slots): ring[(cursor + i) % capacity] = row_i, later rows winning -- of an
    add larger than the ring only the last `capacity` rows are left."""
    i = torch.arange(max(0, n - cap), n, dtype=torch.int64, device="cuda")
    return i, (c0 + i) % cap


def _assert_ring_is_indexed_batch(rb, D, cap, c0, n, obs, nobs, acts, rews, dones, what):
    i, slots = _landing(cap, c0, n)
    assert slots.unique().numel() == slots.numel()
    free = torch.ones(cap, dtype=torch.bool, device="cuda")
    free[slots] = False
    for f, src in (("obs", obs), ("next_obs", nobs)):
        ring = getattr(rb, f).view(torch.int32)
        exp = src.view(torch.int32)[:, :D].index_select(0, i)
        assert torch.equal(ring.index_select(0, slots), exp), (what, f)
        assert bool((ring[free] == STALE).all()), (what, f, "a slot outside the add was written")
    for f, src, stale in (("actions", acts, -7), ("rewards", rews, -7.0), ("dones", dones, 77)):
        ring = getattr(rb, f)
        assert torch.equal(_bits(ring.index_select(0, slots)), _bits(src.index_select(0, i))), (what, f)
        assert bool((ring[free] == stale).all()), (what, f)
    assert rb.size == min(n, cap) and rb.cursor == (c0 + n) % cap, (what, rb.size, rb.cursor)


@gpu
@pytest.mark.parametrize("case", sorted(REPLAY_CASES))
def test_replay_add_on_both_sides_of_its_kernel_bound(case):
    """ReplayBuffer.add_many of f32 rows with the largest row count the fast kernel takes and with one row more
    (drl_replay_add_rows_kernel, at the project's own row widths): either ring is the torch-indexed batch, obs
    and next_obs bit for bit, and on the rows both adds land the two rings are equal.  The add starts from a
    non-zero cursor and wraps the ring; pad floats of a strided batch are NaN and must not arrive; 2050-add adds
    37 rows more than the ring holds."""
    D, div, pad, over, expect = REPLAY_CASES[case]
    Dk = D // div
    below = (2**32 - 1) // (Dk * Dk)
    at = below + 1
    assert below * Dk * Dk < 2**32 <= at * Dk * Dk and below == expect
    if div == 4:    # the 16-B kernel's other conditions (else the float2 kernel's, whose bound is lower still)
        assert D % 4 == 0 and D // 4 >= 2 and (D + pad) % 4 == 0
        assert at * (D // 2) ** 2 >= 2**32       # past add16's bound nothing but the rows kernel is left
    else:
        assert D % 4 != 0 and D // 2 >= 2        # never the 16-B kernel
    stride = D + pad
    extra = 37 if over else 0
    n_max = at + extra
    g = torch.Generator(device="cuda").manual_seed(D)
    obs = torch.rand((n_max, stride), device="cuda", generator=g)
    nobs = torch.rand((n_max, stride), device="cuda", generator=g)
    if pad:
        obs[:, D:] = float("nan")
        nobs[:, D:] = float("nan")
    acts = torch.randint(0, 5, (n_max,), dtype=torch.int32, device="cuda", generator=g)
    rews = torch.rand((n_max,), device="cuda", generator=g)
    dones = (torch.rand((n_max,), device="cuda", generator=g) < 0.3).to(torch.uint8)
    batch = (obs, nobs, acts, rews, dones)
    runs = {}
    for side, rows in (("fast", below), ("rows", at)):
        cap = rows if over else at + 1237          # over: the landing rows are the whole ring
        n = rows + extra
        c0 = cap - 1000                              # the add wraps the ring
        assert min(n, cap) == rows and c0 > 0 and c0 + n > cap
        assert obs[:n].data_ptr() % 16 == 0 and nobs[:n].data_ptr() % 16 == 0
        rb = _replay_run(D, cap, c0, n, *batch)
        assert rb.obs.numel() == cap * D and rb.obs.data_ptr() % 16 == 0 and rb.next_obs.data_ptr() % 16 == 0
        _assert_ring_is_indexed_batch(rb, D, cap, c0, n, *batch, what=(case, side, rows))
        runs[side] = (rb, cap, c0, n)
    # the rows both adds land (the fast add's landing rows; `over`: all but the first of them)
    (ra, cap_a, c0_a, n_a), (rb, cap_b, c0_b, n_b) = runs["fast"], runs["rows"]
    first = max(0, n_a - cap_a, n_b - cap_b)
    i = torch.arange(first, n_a, dtype=torch.int64, device="cuda")
    assert i.numel() >= below - 1
    sa, sb = (c0_a + i) % cap_a, (c0_b + i) % cap_b
    for f in ("obs", "next_obs", "actions", "rewards", "dones"):
        ta, tb = _bits(getattr(ra, f)), _bits(getattr(rb, f))
        assert torch.equal(ta.index_select(0, sa), tb.index_select(0, sb)), (case, f)
    del runs, ra, rb, batch, obs, nobs


# ============================================================== 2. policy-code acts across E * code_bytes = 2^31 ==
# launch_qnet_act_code: a 128 -> 64 net at a 5x5 or 7x7 window takes drl_qnet_act_code4_kernel (a buffer resource
# with 32-bit lane offsets and an (int) record count) while E * code_bytes < 2^31 and drl_qnet_act_code2_kernel at
# and past it; every other net drl_qnet_act_code_kernel (both 64-bit row addresses).  At 9x9 the launch code would
# send a 128 -> 64 net to code2 at every E, but drl_qnet_packed_bytes refuses that net ("the packed network does
# not fit the 160 KB LDS of a CU": layer 0 alone is 128 units x 16 K-slices of hi + lo fragments), so the 9x9 case
# is the widest 9x9 net the suite packs, 96 -> 32, on drl_qnet_act_code_kernel with 192-byte rows.
# v4ok's other conditions hold at 5x5 as at 7x7: layer 0's hi + lo fragments fit the LDS, so lo0_lds with
# frag_off[0] = 0 and frag_lo_off[0] = 8 * code_kt * 64 (qnet_layout), and window <= 7 -- so 5x5 is in.
# (window radius, hidden, side of the bound, DRL_QN_CODE for the pool launch: "2" where the big launch reaches
#  code2 through the bound and the pool launch, far below it, would otherwise take code4)
CODE_CASES = {
    "7x7-128x64-code4-largest": (3, (128, 64), "below", None),
    "7x7-128x64-fallback-code2": (3, (128, 64), "at", "2"),
    "7x7-16x16-generic-2GiB": (3, (16, 16), "at", None),
    "9x9-96x32-generic-2GiB": (4, (96, 32), "at", None),
    "5x5-128x64-code4-largest": (2, (128, 64), "below", None),
    "5x5-128x64-fallback-code2": (2, (128, 64), "at", "2"),
}


@functools.lru_cache(maxsize=None)
def _code_pool(radius):
    """P_POOL real env rows after six steps: (policy code, drone 0's flat observation); built once, only read."""
    from tests.test_policy_code import _env
    env = _env(16, 8, radius, P_POOL, seed=20 + radius)
    code = env.new_code()
    for t in range(6):
        _, _, obs = env.step(env.synth_actions(seed=2, step=t), obs_k=1, code=code)
    env.check_errors()
    return code, obs.reshape(P_POOL, -1).contiguous()


def _sample_envs(E, seed, also=()):
    """2,000 envs: the first 64, the last 64, `also`, the rest seeded at random."""
    rng = np.random.default_rng(seed)
    fixed = np.concatenate([np.arange(64), np.arange(E - 64, E), np.asarray(also, dtype=np.int64)])
    return np.concatenate([fixed, rng.integers(64, E - 64, 2000 - len(fixed))]).astype(np.int64)


def _assert_epilogue_sample(acts, q, sample, eps, seed, step, off, synth_ref):
    from tests.test_dqn import _hash_explore
    s = torch.as_tensor(sample, device="cuda")
    a, qs = acts.index_select(0, s).cpu().numpy(), q.index_select(0, s).cpu()
    greedy = torch.argmax(qs, dim=1).numpy()
    explored = 0
    for k, e in enumerate(sample):
        explores, rnd = _hash_explore(seed, step, off + int(e), q.shape[1], eps)
        explored += explores
        assert a[k, 0] == (rnd if explores else greedy[k]), (int(e), explores)
    assert 0.15 < explored / len(sample) < 0.35     # (epsilon 0.25: both branches are in the sample)
    assert np.array_equal(a[:, 1:], synth_ref.index_select(0, s).cpu().numpy()[:, 1:])


@gpu
@pytest.mark.parametrize("case", list(CODE_CASES))
def test_code_act_on_both_sides_of_2gib_of_codes(case, monkeypatch):
    """QNetwork(input="code").act on a code buffer just below / at 2^31 bytes: every row's Q and greedy action
    equal the pool launch's of the same kernel, and the pool launch is within Q_TOL_EXACT of the host forwards
    of the decoded observation.  Then one launch at epsilon 0.25 with a synth column block and an env_offset for
    which env_offset + e crosses 2^32 inside the launch (include/dronerl.h: the streams hash the 64-bit global
    env index): Q again the pool's on every row, columns 1.. drl_synth_actions' on every row, and on 2,000 envs
    (the first and last 64, the two at the 2^32 crossing, the rest at random) column 0 is the exploration
    stream's draw where the env explores and the argmax of its own Q row elsewhere."""
    from dronerl_amd._native import lib
    from tests.test_policy_code import _nets
    radius, hidden, side, pool_knob = CODE_CASES[case]
    W = 2 * radius + 1
    cb = int(lib().drl_policy_code_bytes(radius))
    below = (2**31 - 1) // cb          # a.E * code_bytes < (1ll << 31)
    at = below + 1
    assert below * cb < 2**31 <= at * cb
    E = below if side == "below" else at
    code_p, x_p = _code_pool(radius)
    cnet, onet = _nets(W * W * 6, hidden, seed=1000 + radius)
    if pool_knob:
        monkeypatch.setenv("DRL_QN_CODE", pool_knob)
    else:
        monkeypatch.delenv("DRL_QN_CODE", raising=False)
    q_p = torch.empty((P_POOL, 5), device="cuda")
    a_p = cnet.act(code_p, epsilon=0.0, q_out=q_p)
    cnet.check_errors()
    monkeypatch.delenv("DRL_QN_CODE", raising=False)   # the big launch picks its kernel from E alone
    _assert_exact_pool_q(onet, q_p, a_p, x_p, case)
    idx = _pool_index(E)
    big = code_p.index_select(0, idx)
    assert big.numel() == E * cb and big.is_contiguous()
    q = torch.empty((E, 5), device="cuda")
    a = cnet.act(big, epsilon=0.0, q_out=q)
    cnet.check_errors()
    _assert_rows_from_pool(q, q_p, idx, f"{case}: Q")
    _assert_rows_from_pool(a, a_p, idx, f"{case}: greedy action")
    del a
    N, eps, seed, step = 3, 0.25, 7, 3
    off = 2**32 - E // 2
    acts = torch.full((E, N), -1, dtype=torch.int32, device="cuda")
    q.fill_(float("nan"))
    cnet.act(big, epsilon=eps, seed=seed, step=step, env_offset=off, actions=acts, q_out=q, synth=(2024, 9))
    cnet.check_errors()
    _assert_rows_from_pool(q, q_p, idx, f"{case}: Q of the exploring launch")
    synth = torch.empty((E, N), dtype=torch.int32, device="cuda")
    assert lib().drl_synth_actions(2024, 9, off, E, N, synth.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(acts[:, 1:], synth[:, 1:])
    _assert_epilogue_sample(acts, q, _sample_envs(E, radius, also=(E // 2 - 1, E // 2)), eps, seed, step, off, synth)
    del big, q, acts, synth, idx


# ================================================================ 4. synthetic actions: the 32- and 64-bit paths ==
@gpu
@pytest.mark.parametrize("N,off", [(64, 0), (63, 0), (63, 2**32 - 400_000)])
def test_synth_actions_fast_and_wide_paths_agree_and_match_the_oracle(N, off):
    """drl_synth_actions with E * N * N just below 2^32 (launch_synth's `fast` multiply-shift path; the constant
    is exact at N = 64 and rounded up at N = 63) and at it (the 64-bit division): the two launches agree on every
    common element, and 5,000 sampled (env, drone) entries of each, the last env's among them, are the oracle's
    counter hash.  The third case starts at an env_offset from which the global env index crosses 2^32."""
    from dronerl_amd._native import lib
    from oracle import oracle
    below = (2**32 - 1) // (N * N)     # (uint64_t)total * N < (1ull << 32), total = E * N
    at = below + 1
    assert below * N * N < 2**32 <= at * N * N
    if N == 64:
        assert (below, at) == (1_048_575, 1_048_576)
    seed, step = 31337, 11
    out = {}
    for E in (below, at):
        o = torch.full((E, N), -1, dtype=torch.int32, device="cuda")
        assert lib().drl_synth_actions(seed, step, off, E, N, o.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        out[E] = o
    torch.cuda.synchronize()
    assert torch.equal(out[at][:below], out[below])
    assert int(out[at].min()) >= 0 and int(out[at].max()) <= 4
    rng = np.random.default_rng(N)
    for E in (below, at):
        envs = np.concatenate([rng.integers(0, E, 5000 - N), np.full(N, E - 1)])
        drones = np.concatenate([rng.integers(0, N, 5000 - N), np.arange(N)])
        flat = torch.as_tensor(envs * N + drones, device="cuda")
        got = out[E].reshape(-1).index_select(0, flat).cpu().numpy()
        want = np.array([oracle.synth_action(seed, step, off + int(e), N, int(d)) for e, d in zip(envs, drones)],
                        dtype=np.int32)
        assert np.array_equal(got, want), (E, np.flatnonzero(got != want)[:8])
    del out


# ============================================================================ 5. get_obs(k) past 4 GiB ==
@gpu
def test_get_obs_rows_past_4gib_match_the_oracle():
    """get_obs(32) of 19,400 envs at grid 64, radius 8 is 19,400 x 221,952 B = 4.31 GB (64-bit row addresses by
    design).  After a seeded reset and three synthetic-action steps the windows of the first 4 envs, the last 16
    and the envs that hold byte offsets 2^31 and 2^32 equal the CPU oracle's, bit for bit; each oracle env runs
    alone at its global index (seed + index, its own row of the action stream)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from oracle import oracle
    from tests.test_gpu_parity import oparams
    p = EnvParams(n_drones=32, grid_size=64, window_radius=8)
    E, k, seed, aseed = 19_400, 32, 5, 9
    row = k * 17 * 17 * 6 * 4
    assert row == 221_952 and E * row > 2**32 + 16 * row
    sel = sorted(set([0, 1, 2, 3, 2**31 // row, 2**32 // row, *range(E - 16, E)]))
    assert sel[4] * row <= 2**31 < (sel[4] + 1) * row and sel[5] * row <= 2**32 < (sel[5] + 1) * row
    env = BatchedDeliveryDrones(p, E)
    env.reset(seed=seed)
    for t in range(1, 4):
        env.step(env.synth_actions(seed=aseed, step=t))
    obs = env.get_obs(k)
    assert obs.numel() * 4 == E * row
    got = obs.index_select(0, torch.as_tensor(sel, device="cuda")).cpu().numpy()
    env.check_errors()
    o = oracle.OracleMulti(oparams(p), len(sel))
    o.reset(seed + np.asarray(sel))
    for t in range(1, 4):
        o.step(oracle.synth_actions(aseed, t, sel, p.n_drones))
    want = o.obs(8, k)
    assert float(want[..., 4].max()) > 0
    for j, e in enumerate(sel):
        assert np.array_equal(got[j].view(np.uint32), want[j].view(np.uint32)), f"env {e}"
    del obs, env


# =================================== 3. f32-observation acts between 2 and 4 GiB, the refusal, rows past 4 GiB ==
# (last in the file: the 4.35 GB buffer lives until the module's tests are done)
OBS_ROWS, OBS_D = 3_700_000, 294


@pytest.fixture(scope="module")
def big_obs():
    """(pool [P_POOL, 294] randn, big [3,700,000, 294] with big[e] = pool[h(e)], h): 4.35 GB, only read."""
    g = torch.Generator().manual_seed(294)
    pool = torch.randn((P_POOL, OBS_D), generator=g).cuda()
    idx = _pool_index(OBS_ROWS)
    big = pool.index_select(0, idx)
    assert big.numel() * 4 == OBS_ROWS * OBS_D * 4 > 2**32
    yield pool, big, idx
    del pool, big, idx
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _dense_net(precision):
    from dronerl_amd.dqn import QNetwork
    g = torch.Generator().manual_seed(77)
    net = QNetwork(OBS_D, (128, 64), generator=g, precision=precision)
    for b in net.biases:
        b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    net.pack()
    return net


def _dense_pool_run(precision, pool):
    """The pool launch of drl_qnet_act (f32: drl_qnet_act_f32_kernel, bf16: drl_qnet_act_kernel), checked against
    the host as tests/test_qnet_descriptor_space.py checks these kernels."""
    from tests.test_dqn import Q_TOL_BF16, Q_TOL_F32
    net = _dense_net(precision)
    q_p = torch.empty((P_POOL, 5), device="cuda")
    a_p = net.act(pool, epsilon=0.0, q_out=q_p)
    net.check_errors()
    if precision == "f32":
        _assert_exact_pool_q(net, q_p, a_p, pool, "drl_qnet_act f32")
    else:
        ref, ref32 = net.reference_q(pool, bf16_operands=True), net.reference_q(pool)
        e16 = ((q_p - ref).abs() / (1 + ref.abs())).max().item()
        e32 = ((q_p - ref32).abs() / (1 + ref32.abs())).max().item()
        print(f"drl_qnet_act bf16: pool err vs bf16-operand forward {e16:.3e}, vs f32 {e32:.3e}")
        assert e16 <= Q_TOL_BF16, e16
        assert e32 <= Q_TOL_F32, e32
        assert torch.equal(a_p[:, 0].long(), torch.argmax(q_p, dim=1))
        top2 = torch.topk(ref, 2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > 2 * Q_TOL_BF16 * (1 + top2[:, 0].abs())
        assert safe.float().mean().item() > 0.5
        assert torch.equal(a_p[safe, 0].long(), torch.argmax(ref, dim=1)[safe])
    return net, q_p, a_p


def _largest_accepted(stride):
    """The largest E that qnet_act_impl accepts: num_envs * obs_stride * 4 < 2^32."""
    E = (2**32 - 1) // (stride * 4)
    assert E * stride * 4 < 2**32 <= (E + 1) * stride * 4
    return E


@gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_obs_act_on_the_largest_accepted_buffer(precision, big_obs):
    """drl_qnet_act on 3,652,183 rows of 294 floats, 4,294,967,208 bytes: the row offsets are uint32 and, in the
    f32 kernel, cast to (int) for the buffer loads together with the record count; from row 1,826,091 (which
    straddles byte 2^31) on both casts are negative.  Every row's Q and action equal the pool launch's."""
    pool, big, idx = big_obs
    E = _largest_accepted(OBS_D)
    assert E == 3_652_183 and E * OBS_D * 4 == 4_294_967_208
    assert 1_826_091 * OBS_D * 4 < 2**31 < 1_826_092 * OBS_D * 4
    net, q_p, a_p = _dense_pool_run(precision, pool)
    q = torch.empty((E, 5), device="cuda")
    a = net.act(big[:E], epsilon=0.0, q_out=q)
    net.check_errors()
    _assert_rows_from_pool(q, q_p, idx[:E], f"{precision}: Q")
    _assert_rows_from_pool(a, a_p, idx[:E], f"{precision}: action")


@gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_obs_act_on_every_second_row_up_to_4gib(precision, big_obs):
    """The same buffer with obs_stride = 588 (every second row: the act on one column of a strided
    observation), E = 1,826,091, the largest the guard accepts at this stride."""
    pool, big, idx = big_obs
    E = _largest_accepted(2 * OBS_D)
    assert E == 1_826_091 and 2 * E <= OBS_ROWS
    net, q_p, a_p = _dense_pool_run(precision, pool)
    obs = big[:2 * E:2]
    assert obs.shape[0] == E and obs.stride(0) == 2 * OBS_D and obs.data_ptr() == big.data_ptr()
    q = torch.empty((E, 5), device="cuda")
    a = net.act(obs, epsilon=0.0, q_out=q)
    net.check_errors()
    even = idx[:2 * E:2].contiguous()
    _assert_rows_from_pool(q, q_p, even, f"{precision} stride 588: Q")
    _assert_rows_from_pool(a, a_p, even, f"{precision} stride 588: action")


@gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_obs_act_refuses_4gib(precision, big_obs):
    """One row more on the same pointer: the "4 GiB" error before any device work (the actions stay as they
    were)."""
    from dronerl_amd._native import DroneRLError
    _, big, _ = big_obs
    E = _largest_accepted(OBS_D) + 1
    assert E == 3_652_184
    net = _dense_net(precision)
    acts = torch.full((E, 1), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(DroneRLError, match="4 GiB"):
        net.act(big[:E], epsilon=0.0, actions=acts)
    torch.cuda.synchronize()
    assert bool((acts == -1).all())
    net.check_errors()


@gpu
def test_conv_act_rows_past_4gib(big_obs):
    """ConvQNetwork (tests/test_convnet.py's net "b", 7x7) on all 3,700,000 rows: 64-bit row addresses by design,
    the rows from 3,652,184 on start past byte 2^32."""
    from dronerl_amd.dqn import ConvQNetwork
    from tests.test_convnet import NETS, Q_TOL_EXACT, _host_q, _params
    pool, big, idx = big_obs
    W, conv, dense = NETS["b"]
    params = _params(W, conv, dense, seed=98)
    net = ConvQNetwork((W, W, 6), conv, dense)
    net.load(*params)
    q_p = torch.empty((P_POOL, 5), device="cuda")
    a_p = net.act(pool, 0.0, q_out=q_p)
    net.check_errors()
    x = pool.cpu().reshape(P_POOL, W, W, 6)
    ref32, ref64 = _host_q(params, conv, x, torch.float32), _host_q(params, conv, x, torch.float64)
    scale = 1 + ref32.abs().max(dim=1, keepdim=True).values
    err32 = ((q_p.cpu() - ref32).abs() / scale).max().item()
    err64 = ((q_p.cpu().double() - ref64).abs() / scale.double()).max().item()
    print(f"conv b: pool err vs f32 {err32:.3e}, vs f64 {err64:.3e}")
    assert err32 <= Q_TOL_EXACT and err64 <= Q_TOL_EXACT, (err32, err64)
    assert torch.equal(a_p[:, 0].long(), torch.argmax(q_p, dim=1))
    q = torch.empty((OBS_ROWS, 5), device="cuda")
    a = net.act(big, 0.0, q_out=q)
    net.check_errors()
    _assert_rows_from_pool(q, q_p, idx, "conv: Q")
    _assert_rows_from_pool(a, a_p, idx, "conv: action")


@gpu
def test_wide_act_rows_past_4gib(big_obs):
    """WideQNetwork 294 -> 256-128-64 on all 3,700,000 rows (64-bit row addresses by design)."""
    from dronerl_amd.dqn import WideQNetwork
    pool, big, idx = big_obs
    g = torch.Generator().manual_seed(256)
    net = WideQNetwork(OBS_D, (256, 128, 64), generator=g)
    for b in net.biases:
        b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    net.pack()
    q_p = torch.empty((P_POOL, 5), device="cuda")
    a_p = net.act(pool, 0.0, q_out=q_p)
    net.check_errors()
    _assert_exact_pool_q(net, q_p, a_p, pool, "wide 256-128-64")
    q = torch.empty((OBS_ROWS, 5), device="cuda")
    a = net.act(big, 0.0, q_out=q)
    net.check_errors()
    _assert_rows_from_pool(q, q_p, idx, "wide: Q")
    _assert_rows_from_pool(a, a_p, idx, "wide: action")


# ===================================================================== 6. the manifest of size bounds (no GPU) ==
# Every line of dronerl_amd/csrc/** that holds `<< 31`, `<< 32` or `4 GiB`: (file, stripped line) -> the test of
# this file that runs the bound from both sides ("test_..."), another file's test that pins a host refusal
# ("file.py::test_..."), or "-- reason" for a line that bounds no launch.
_T = "test_size_thresholds.py::"
_CAP = ("a replay slot index is an int32 field; the refusal's message and its lower side (capacity 0) are pinned "
        "before any device work by ")
_MAGIC = "-- the multiply-shift constant ceil(2^32 / d) itself, no bound (its exactness bound is the launch's)"
SIZE_BOUNDS = {
    ("dronerl_qnet.hip", "// the observation rows by buffer loads (32-bit offsets; the host checks obs < 4 GiB)"):
        _T + "test_obs_act_on_the_largest_accepted_buffer",
    ("dronerl_qnet.hip", "a.E * (int64_t)lay::code_bytes(window) < (1ll << 31);"):
        _T + "test_code_act_on_both_sides_of_2gib_of_codes",
    ("dronerl_qnet.hip",
     "al16(a.next_obs) && al16(a.buf_obs) && al16(a.buf_next_obs) && total4 * D4 < (1ull << 32)) {"):
        _T + "test_replay_add_on_both_sides_of_its_kernel_bound",
    ("dronerl_qnet.hip",
     "} else if (D2 >= 2 && total * D2 < (1ull << 32)) {  // multiply-shift row index exact (FastDiv bound)"):
        _T + "test_replay_add_on_both_sides_of_its_kernel_bound",
    ("dronerl_qnet_api.cpp",
     'if (num_envs * obs_stride * 4 >= ((int64_t)1 << 32)) return fail("obs larger than 4 GiB (32-bit row offsets)");'):
        _T + "test_obs_act_refuses_4gib",
    ("dronerl_kernels.hip", "const int fast = (uint64_t)total * (uint64_t)N < (1ull << 32) ? 1 : 0;"):
        _T + "test_synth_actions_fast_and_wide_paths_agree_and_match_the_oracle",
    ("dronerl_kernels.hip", "twist_wave(reinterpret_cast<uint32_t*>((hi << 32) | lo), lane);"):
        "-- a 64-bit pointer put together from two 32-bit halves, no bound",
    ("dronerl_learn.hip",
     "__hip_atomic_store((gu64*)g, ((uint64_t)epoch << 32) | __float_as_uint(v), __ATOMIC_RELAXED,"):
        "-- layout of a hand-off granule (epoch tag in the high word), no bound",
    ("dronerl_internal.h", "f.m = f.one ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);"): _MAGIC,
    ("widenet/dronerl_widenet_layout.h",
     "inline int32_t fastdiv_magic(int d) { return d > 1 ? (int32_t)(uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0; }"):
        _MAGIC,
    ("convnet/dronerl_convnet_layout.h",
     "inline int32_t fastdiv_magic(int d) { return d > 1 ? (int32_t)(uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0; }"):
        _MAGIC,
}
# the one capacity refusal of every learner, population, league and self-play call (check_ring)
SIZE_BOUNDS[("dronerl_learn_args.h",
             'if (r->capacity < 1 || r->capacity >= ((int64_t)1 << 31)) return "replay capacity must be in [1, 2^31)";')] = (
    "-- " + _CAP + "test_large_batch_learner.py::test_large_calls_validate_before_device_work")
_ENVS_LINE = "if (num_envs < 1 || num_envs * n_drones >= ((int64_t)1 << 31))"
for _f, _t in {
    "league/dronerl_league_api.cpp": "test_league.py::test_league_calls_validate_before_device_work",
    "convleague/dronerl_convleague_api.cpp": "test_conv_league.py::test_convleague_calls_validate_before_device_work",
    "selfplay/dronerl_selfplay_api.cpp": "test_selfplay.py::test_selfplay_calls_validate_before_device_work",
    "convselfplay/dronerl_convselfplay_api.cpp": "test_conv_selfplay.py::test_convselfplay_act_validates_before_device_work",
}.items():
    SIZE_BOUNDS[(_f, _ENVS_LINE)] = _t     # host refusal, pinned at num_envs = 2^29 with 4 drones
SIZE_BOUNDS[("convselfplay/dronerl_convselfplay_api.cpp", "if ((int64_t)team * num_envs >= ((int64_t)1 << 31))")] = (
    "-- host refusal of a learner's int32 row index; with team <= n_drones it is implied by the num_envs * n_drones "
    "refusal one line above, pinned by test_conv_selfplay.py::test_convselfplay_act_validates_before_device_work")
_MEMBERS_LINE = "if (envs_per_member < 1 || envs_per_member * members >= ((int64_t)1 << 31))"
for _f, _t in {
    "population/dronerl_population_api.cpp": "test_population.py::test_population_calls_validate_before_device_work",
    "convpop/dronerl_convpop_api.cpp": "test_conv_population.py::test_convpop_calls_validate_before_device_work",
}.items():
    SIZE_BOUNDS[(_f, _MEMBERS_LINE)] = ("-- host refusal of an int32 global env index (members <= 1024); its message "
                                        "and lower side (envs_per_member 0) are pinned by " + _t)


def _size_bound_lines(csrc):
    found = set()
    for f in glob.glob(os.path.join(csrc, "**", "*"), recursive=True):
        if os.path.isfile(f) and f.endswith((".hip", ".cpp", ".h")):
            for line in open(f, encoding="utf-8"):
                if "<< 31" in line or "<< 32" in line or "4 GiB" in line:
                    found.add((os.path.relpath(f, csrc).replace(os.sep, "/"), line.strip()))
    return found


def test_every_size_bound_is_listed_with_its_test():
    """A launch bound that is new, or whose text changed, fails here until SIZE_BOUNDS lists it with the test
    that runs it at the bound or the reason it needs none; a listed test must exist."""
    found = _size_bound_lines(os.path.join(REPO, "dronerl_amd", "csrc"))
    listed = set(SIZE_BOUNDS)
    assert found == listed, {"not listed": sorted(found - listed), "no longer in the source": sorted(listed - found)}
    for key, ref in SIZE_BOUNDS.items():
        if ref.startswith("-- "):
            assert len(ref) > 20, key
            refs = re.findall(r"(test_\w+\.py)::(test_\w+)", ref)
        else:
            refs = re.findall(r"^(test_\w+\.py)::(test_\w+)$", ref)
            assert refs, (key, ref)
        for fname, test in refs:
            text = open(os.path.join(REPO, "tests", fname), encoding="utf-8").read()
            assert re.search(rf"^def {test}\(", text, re.M), (key, fname, test)
