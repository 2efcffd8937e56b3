"""Reference of the conv DQN learner's tests (tests/test_convnet_learner.py):
a torch restatement of one train_jax.py learner block (:68-98) for a
ConvQNetwork -- the forward of tests/test_convnet.py::_host_q, autograd for
the gradient, optax's Adam formula written out as in
tests/test_dqn_learner.py::_torch_step -- run in float64 and in float32.

The device is compared with the f64 restatement; how far it may be from it
comes from the f32 restatement alone (`tolerance`): per step and tensor
max(1e-5, 4 x the f32 restatement's own distance from the f64 one on that
step).  1e-5 is the dense learner test's figure; the factor 4 allows the
device's different summation order on top of f32 rounding.  It is needed
because Adam's first steps turn a tiny gradient into an update of almost
+-lr, which amplifies rounding: with synthetic windows the f32-to-f64
distance alone reaches 7e-6 at the first step from zero moments.
"""
import numpy as np
import torch


def _c(out_channels, kernel_size, stride, padding):
    return {"out_channels": out_channels, "kernel_size": kernel_size, "stride": stride, "padding": padding}


# case -> (W, conv layers, dense widths)
NETS = {
    "a": (7, (_c(4, 3, 1, 1),), (8,)),                                    # the reference's dqn-agent-5 shape
    "b": (7, (_c(8, 3, 1, 1),), ()),                                      # train_jax's default; zero biases
    "c": (9, (_c(8, 3, 1, 0), _c(12, 3, 2, 1)), (16, 8)),                 # two conv layers, stride 2
    "e": (3, (_c(32, 1, 1, 0),), (8,)),                                   # 1x1 kernel, widest Cout; f32 rows only
    "f": (7, (_c(6, 2, 3, 0),), ()),                                      # even kernel, stride 3, uncovered inputs
    "g": (5, (_c(5, 5, 1, 2),), (128,)),                                  # K = 150, widest dense
    "h": (9, (_c(8, 3, 1, 1), _c(8, 3, 2, 0), _c(16, 2, 1, 0)), ()),      # three conv layers
    "i": (7, (_c(5, 3, 1, 1), _c(7, 2, 3, 0)), (8,)),                     # layer 1 leaves positions of layer 0 uncovered
}

# (case, rows, batch, hyperparameters, ring slots): the per-step parity cases
CASES = [
    ("b", "code", 8, {}, 300),
    ("a", "obs", 1, dict(epsilon_decay=0.9, epsilon_decay_every=1), 300),
    ("c", "code", 5, dict(tau=0.6, target_update_interval=3), 300),
    ("f", "obs", 64, {}, 96),
    ("e", "obs", 8, {}, 300),
    ("g", "code", 16, dict(learning_rate=3e-3), 300),
    ("h", "code", 8, {}, 300),
    ("i", "obs", 8, {}, 300),
]
CASE_IDS = [f"{c[0]}-{c[1]}-{c[2]}" for c in CASES]


def rel(a, b):
    """oracle/dqn_learner.py's / tests/test_dqn_learner.py's _rel."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (1e-3 + np.max(np.abs(b))))


def tolerance(f32_value, f64_value):
    return max(1e-5, 4.0 * rel(f32_value, f64_value))


def shapes(W, conv, dense, n_actions=5):
    """[(weight shape, bias shape)] in forward order: conv layers, dense layers, the Q head."""
    out, side, cin = [], W, 6
    for c in conv:
        k, co = c["kernel_size"], c["out_channels"]
        out.append(((co, cin, k, k), (co,)))
        side, cin = (side + 2 * c["padding"] - k) // c["stride"] + 1, co
    sizes = [side * side * cin, *dense, n_actions]
    for i in range(len(sizes) - 1):
        out.append(((sizes[i + 1], sizes[i]), (sizes[i + 1],)))
    return out


def random_params(W, conv, dense, seed, bias_std=0.05):
    """Seeded f32 parameters [(W, b)]: lecun-normal weights, biases ~ N(0, bias_std) (0: zeros, flax's init)."""
    g = np.random.default_rng(seed)
    out = []
    for ws, bs in shapes(W, conv, dense):
        fan_in = int(np.prod(ws[1:]))
        b = g.normal(0, bias_std, bs) if bias_std else np.zeros(bs)
        out.append((g.normal(0, (1.0 / fan_in) ** 0.5, ws).astype(np.float32), b.astype(np.float32)))
    return out


def synthetic_windows(W, n, seed):
    """Windows f32 [n, W*W*6] as the env writes them: sparse 0/1 channels, the charge channel k/100."""
    g = np.random.default_rng(seed)
    x = (g.random((n, W * W, 6)) < 0.15).astype(np.float32)
    x[:, :, 4] *= g.integers(0, 101, (n, W * W)).astype(np.float32) / np.float32(100)
    return x.reshape(n, W * W * 6)


def forward(ps, conv, x):
    """tests/test_convnet.py::_host_q on a flat parameter list [w0, b0, w1, b1, ...]; x [B, W, W, 6]."""
    h = x.permute(0, 3, 1, 2)
    for i, c in enumerate(conv):
        h = torch.relu(torch.nn.functional.conv2d(h, ps[2 * i], ps[2 * i + 1], stride=c["stride"],
                                                  padding=c["padding"]))
    h = h.flatten(1)
    rest = ps[2 * len(conv):]
    for i in range(0, len(rest), 2):
        h = h @ rest[i].t() + rest[i + 1]
        if i < len(rest) - 2:
            h = torch.relu(h)
    return h


def ref_step(st, hp, W, conv, X, Xn, act, rew, done, dtype, trained=True):
    """One learner block in `dtype` from the f32 state `st` = {"online", "target", "m", "v": [(W, b)], "step",
    "count"}: returns the new sets (numpy, `dtype`) and the loss.  hp: an object with gamma, learning_rate,
    beta1, beta2, adam_eps, tau, target_update_interval (oracle.dqn_learner.HParams)."""
    flat = lambda k: [torch.tensor(np.asarray(t), dtype=dtype) for wb in st[k] for t in wb]  # noqa: E731
    pair = lambda xs: [(xs[i], xs[i + 1]) for i in range(0, len(xs), 2)]  # noqa: E731
    online, target, m, v = flat("online"), flat("target"), flat("m"), flat("v")
    loss = 0.0
    if trained:
        ps = [p.clone().requires_grad_() for p in online]
        B = X.shape[0]
        q = forward(ps, conv, torch.tensor(X, dtype=dtype).reshape(B, W, W, 6))
        qa = q.gather(1, torch.tensor(act, dtype=torch.long)[:, None])[:, 0]
        with torch.no_grad():
            mx = forward(target, conv, torch.tensor(Xn, dtype=dtype).reshape(B, W, W, 6)).max(dim=1).values
            td = torch.tensor(rew, dtype=dtype) + hp.gamma * mx * (1 - torch.tensor(done, dtype=dtype))
        lo = ((qa - td) ** 2).mean()
        lo.backward()
        loss = float(lo.detach())
        t = st["count"] + 1
        new_p, new_m, new_v = [], [], []
        for p, mm, vv in zip(ps, m, v):
            g = p.grad
            mm = (1 - hp.beta1) * g + hp.beta1 * mm
            vv = (1 - hp.beta2) * g * g + hp.beta2 * vv
            u = (mm / (1 - hp.beta1 ** t)) / (torch.sqrt(vv / (1 - hp.beta2 ** t)) + hp.adam_eps)
            new_p.append(p.detach() - hp.learning_rate * u)
            new_m.append(mm)
            new_v.append(vv)
        online, m, v = new_p, new_m, new_v
    if st["step"] % hp.target_update_interval == 0:
        target = [hp.tau * o + (1 - hp.tau) * t_ for o, t_ in zip(online, target)]
    num = lambda xs: pair([x.numpy() for x in xs])  # noqa: E731
    return {"online": num(online), "target": num(target), "m": num(m), "v": num(v), "loss": loss}
