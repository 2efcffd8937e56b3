"""A float32 numpy restatement of the conv learners' per-row forward
(dronerl_amd/csrc/convlearn/dronerl_convlearn_rows.h `cl_forward`) in its own
summation order: the yardstick of the conv population's act
(tests/test_conv_population.py), whose Q must equal it bit for bit.

Every product and every sum is rounded to f32 on its own (numpy float32
arithmetic; the device code is compiled without FMA contraction).
  conv output (co, oy, ox): z = 0; for ci, ky, kx in that order, skipping taps
    outside the map, z = z + w * v; then + bias; relu.
  dense unit: lane c of 64 sums k = c, c + 64, ... in order from 0.0; then for
    m = 1, 2, 4, ..., 32 all lanes do s[c] = s[c] + s[c ^ m]; z = s[0] + bias.
  layer 0 reads the observation's [y][x][c], later layers the previous
    layer's [c][y][x]; the flatten is the identity; relu everywhere but the
    Q head.
"""
import numpy as np

F = np.float32


def _relu(z):
    return np.where(z > 0, z, F(0)).astype(F)


def _conv(x, w, b, c, side, first):
    """x [n, ...] (first: [y][x][c] flat, else [ci][y][x] flat) -> [n, co * os * os]."""
    n = x.shape[0]
    co, cin, k, _ = w.shape
    s, p = c["stride"], c["padding"]
    os_ = (side + 2 * p - k) // s + 1
    xv = x.reshape(n, side, side, cin) if first else x.reshape(n, cin, side, side)
    oy = np.arange(os_)
    z = np.zeros((n, co, os_, os_), F)
    for ci in range(cin):
        for ky in range(k):
            iy = oy * s + ky - p
            oky = (iy >= 0) & (iy < side)
            iyc = np.clip(iy, 0, side - 1)
            for kx in range(k):
                ix = oy * s + kx - p
                okx = (ix >= 0) & (ix < side)
                ixc = np.clip(ix, 0, side - 1)
                v = xv[:, iyc][:, :, ixc, ci] if first else xv[:, ci][:, iyc][:, :, ixc]  # [n, os, os]
                term = (w[None, :, ci, ky, kx, None, None].astype(F) * v[:, None].astype(F)).astype(F)
                inside = (oky[:, None] & okx[None, :])[None, None]
                z = np.where(inside, (z + term).astype(F), z)
    z = (z + b[None, :, None, None].astype(F)).astype(F)
    return z.reshape(n, co * os_ * os_), os_


def _dense(x, w, b):
    """x [n, K], w [J, K] -> z [n, J] (no relu)."""
    n, K = x.shape
    J = w.shape[0]
    lanes = np.arange(64)
    s = np.zeros((n, J, 64), F)
    for i in range((K + 63) // 64):
        kk = i * 64 + lanes
        ok = kk < K
        kc = np.minimum(kk, K - 1)
        term = (w[None, :, kc].astype(F) * x[:, None, kc].astype(F)).astype(F)
        s = np.where(ok[None, None], (s + term).astype(F), s)
    m = 1
    while m < 64:
        s = (s + s[:, :, lanes ^ m]).astype(F)
        m <<= 1
    return (s[:, :, 0] + b[None].astype(F)).astype(F)


def forward(params, conv, x, W):
    """Q [n, A] float32.  params: [(W, b)] in forward order (conv layers
    [out][in][k][k], dense [out][in], the Q head last), float32 arrays; conv:
    the conv layers' dicts; x: float32 [n, W*W*6] windows."""
    h = np.ascontiguousarray(x, F).reshape(x.shape[0], -1)
    side = W
    for i, c in enumerate(conv):
        w, b = params[i]
        h, side = _conv(h, np.asarray(w, F), np.asarray(b, F), c, side, i == 0)
        h = _relu(h)
    rest = params[len(conv):]
    for i, (w, b) in enumerate(rest):
        h = _dense(h, np.asarray(w, F), np.asarray(b, F))
        if i + 1 < len(rest):
            h = _relu(h)
    return h
