"""TEST INFRASTRUCTURE ONLY: a numpy restatement of one learner step with the
Double DQN target (include/dronerl.h drl_dqn_double_train and the calls
beside it), built from the oracle's own pieces (oracle/dqn_learner.py
forward, backprop4, _adam, sample_indices, decode_code_rows).

``double_step`` is oracle.learner_step's block -- or, with ``weights``,
tests/_per_ref.per_step's -- with one change in the TD rule:

    qs = Q_online(next_obs_b)      (the online parameters the step started with)
    a* = 0; for j = 1 .. A-1: if qs[j] > qs[a*]: a* = j
    td = r + (gamma * qt[a*]) * (1 - done)

With ``double=False`` it takes max_a qt and reproduces oracle.learner_step /
_per_ref.per_step bit for bit (tests/test_double_dqn.py pins that on the CPU),
so the restatement cannot drift from the oracle where the two rules coincide.
"""
from __future__ import annotations

import numpy as np

from oracle import dqn_learner as O

F = np.float32


def select(qs_row: np.ndarray) -> int:
    """jnp.argmax: the first maximum; a NaN never wins a comparison."""
    a = 0
    for j in range(1, qs_row.shape[0]):
        if qs_row[j] > qs_row[a]:
            a = j
    return a


def double_step(st: O.LearnerState, hp: O.HParams, obs, next_obs, actions, rewards, dones, size: int, slots=None,
                weights=None, code_window: int = 0, double: bool = True) -> dict:
    """One learner step on the rows `slots` (None: the uniform draw at
    st.step) with the importance weights `weights` (None: unweighted, the
    uniform learner's expressions).  Updates `st` in place.  info: trained,
    rows, loss, absd (|d| of the rows), qs / qt (the selector's and the
    target's next-state values), sel (a* per row)."""
    step = st.step
    info = {"trained": size >= hp.batch, "rows": None, "loss": F(0.0), "absd": None}
    if size >= hp.batch:
        idx = O.sample_indices(hp.sample_seed, step, hp.batch, size) if slots is None else [int(s) for s in slots]
        info["rows"] = idx
        w = None if weights is None else np.asarray(weights, F)
        n_in = st.online[0][0].shape[1]
        if code_window:
            X = O.decode_code_rows(obs[idx], code_window)
            Xn = O.decode_code_rows(next_obs[idx], code_window)
        else:
            X = obs[idx, :n_in].astype(F)
            Xn = next_obs[idx, :n_in].astype(F)
        zs, hs, q = O.forward(st.online, X)
        _, _, qt = O.forward(st.target, Xn)
        _, _, qs = O.forward(st.online, Xn)  # the selector: no gradient flows through it
        B, A = hp.batch, q.shape[1]
        d = np.zeros(B, F)
        act = np.zeros(B, np.int64)
        sel = np.zeros(B, np.int64)
        for b in range(B):
            s = idx[b]
            if double:
                sel[b] = select(qs[b])
                nxt = qt[b, sel[b]]
            else:
                nxt = qt[b, 0]
                for j in range(1, A):
                    nxt = qt[b, j] if qt[b, j] > nxt else nxt
            notdone = F(0.0) if dones[s] else F(1.0)
            td = F(rewards[s]) + (F(hp.gamma) * nxt) * notdone
            a = int(actions[s])
            ok = 0 <= a < A
            d[b] = (q[b, a] if ok else td) - td
            act[b] = a if ok else -1
        loss = F(0.0)
        for b in range(B):
            loss = F(loss + (d[b] * d[b] if w is None else w[b] * (d[b] * d[b])))
        loss = F(loss / F(B))
        D = np.zeros((B, A), F)
        for b in range(B):
            if act[b] >= 0:
                g = (d[b] + d[b]) / F(B)
                D[b, act[b]] = g if w is None else w[b] * g
        st.beta1_pow *= hp.beta1
        st.beta2_pow *= hp.beta2
        bc1, bc2 = F(1.0 - st.beta1_pow), F(1.0 - st.beta2_pow)
        L = len(st.online)
        deltas = [None] * L
        deltas[L - 1] = D
        for l in range(L - 1, 0, -1):
            dh = O.backprop4(deltas[l], st.online[l][0])
            deltas[l - 1] = np.where(hs[l - 1] > 0, dh, F(0.0)).astype(F)
        inputs = [X] + hs
        new_online, new_m, new_v = [], [], []
        for l in range(L):
            wl, bl = st.online[l]
            gw, gb = np.zeros_like(wl), np.zeros_like(bl)
            for r in range(B):
                gw = gw + deltas[l][r][:, None] * inputs[l][r][None, :]
                gb = gb + deltas[l][r]
            w2, mw2, vw2 = O._adam(hp, wl, gw, st.m[l][0], st.v[l][0], bc1, bc2)
            b2, mb2, vb2 = O._adam(hp, bl, gb, st.m[l][1], st.v[l][1], bc1, bc2)
            new_online.append((w2, b2))
            new_m.append((mw2, mb2))
            new_v.append((vw2, vb2))
        st.online, st.m, st.v = new_online, new_m, new_v
        st.count += 1
        info.update(loss=loss, absd=np.abs(d), qs=qs, qt=qt, sel=sel)
    st.loss = info["loss"]
    if step % hp.target_update_interval == 0:
        tau, omt = F(hp.tau), F(1.0 - hp.tau)
        st.target = [((tau * w_ + omt * tw).astype(F), (tau * b_ + omt * tb).astype(F))
                     for (w_, b_), (tw, tb) in zip(st.online, st.target)]
    if step % hp.epsilon_decay_every == 0:
        e = F(st.epsilon * F(hp.epsilon_decay))
        st.epsilon = e if e > F(hp.epsilon_end) else F(hp.epsilon_end)
    st.step = step + 1
    return info
