"""Reference of the prioritized conv learner's tests (tests/test_conv_per.py):
tests/_conv_learner_ref.py's ref_step -- a torch restatement of one
train_jax.py learner block for a ConvQNetwork, autograd for the gradient,
optax's Adam written out -- with the rows' importance weights in the loss,
mean(w * (q_a - td)^2), run in float64 and in float32.  It also returns the
rows' |q_a - td|, from which the new priorities are formed.  The tree, the
draw, the weights and the priorities are tests/_per_ref.py's, as it is.
"""
import numpy as np
import torch

from tests._conv_learner_ref import forward


def ref_step(st, hp, W, conv, X, Xn, act, rew, done, weights, dtype, trained=True):
    """One learner block in `dtype` from the f32 state `st` = {"online", "target", "m", "v": [(W, b)], "step",
    "count"} on the given rows with importance weights `weights` (f32 [B]): returns the new sets (numpy, `dtype`),
    the loss and "absd", the rows' |q_a - td| (numpy, `dtype`; None without a sample)."""
    flat = lambda k: [torch.tensor(np.asarray(t), dtype=dtype) for wb in st[k] for t in wb]  # noqa: E731
    pair = lambda xs: [(xs[i], xs[i + 1]) for i in range(0, len(xs), 2)]  # noqa: E731
    online, target, m, v = flat("online"), flat("target"), flat("m"), flat("v")
    loss, absd = 0.0, None
    if trained:
        ps = [p.clone().requires_grad_() for p in online]
        B = X.shape[0]
        q = forward(ps, conv, torch.tensor(X, dtype=dtype).reshape(B, W, W, 6))
        qa = q.gather(1, torch.tensor(act, dtype=torch.long)[:, None])[:, 0]
        with torch.no_grad():
            mx = forward(target, conv, torch.tensor(Xn, dtype=dtype).reshape(B, W, W, 6)).max(dim=1).values
            td = torch.tensor(rew, dtype=dtype) + hp.gamma * mx * (1 - torch.tensor(done, dtype=dtype))
        w = torch.tensor(np.asarray(weights, np.float32), dtype=dtype)
        lo = (w * (qa - td) ** 2).mean()
        lo.backward()
        loss = float(lo.detach())
        absd = (qa - td).detach().abs().numpy()
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
    return {"online": num(online), "target": num(target), "m": num(m), "v": num(v), "loss": loss, "absd": absd}
