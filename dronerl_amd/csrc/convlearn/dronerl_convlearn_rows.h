// dronerl_convlearn_rows.h — the per-row forward and backward of the conv learners, shared by
// convlearn/dronerl_convlearn.hip (batches up to 64) and convlarge/dronerl_convlarge.hip (batches up to 4096), in
// the manner of dronerl_learn_common.h: both rows kernels include it, so a row's activations and deltas cannot
// drift apart between the two families.  A workgroup holds one row (input, every layer's relu(z) and dL/dz) in
// LDS, laid out by the validated plan (dronerl_convlearn_layout.h); every thread of it calls these and puts a
// barrier between two layers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronerl_convlearn_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the dense learner
#pragma clang fp contract(off)

namespace drl {
namespace cl {

namespace {

// Layer l's forward on the row in LDS: relu(z) to its act words (the Q head: z to its delta words).
__device__ __forceinline__ void cl_forward(const Plan& P, int l, const float* __restrict__ W, float* row) {
    const LLayer& q = P.l[l];
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* w = W + q.woff;
    const float* bias = W + q.boff;
    const float* x = row + q.in;
    float* out = row + (q.act >= 0 ? q.act : q.delta);
    const bool relu = q.act >= 0;
    if (q.conv) {
        const int os = q.out_side, is = q.in_side, hw = os * os, k = q.k;
        for (int e = tid; e < q.n_out; e += nt) {
            const int co = e / hw, pos = e - co * hw, oy = pos / os, ox = pos - oy * os;
            const float* wc = w + (int64_t)co * q.K;
            float z = 0.0f;
            for (int ci = 0; ci < q.cin; ++ci)
                for (int ky = 0; ky < k; ++ky) {
                    const int iy = oy * q.s + ky - q.p;
                    if (iy < 0 || iy >= is) continue;
                    for (int kx = 0; kx < k; ++kx) {
                        const int ix = ox * q.s + kx - q.p;
                        if (ix < 0 || ix >= is) continue;
                        // layer 0 reads the observation's [y][x][c]; later layers the previous [c][y][x]
                        const float v = l == 0 ? x[(iy * is + ix) * 6 + ci] : x[(ci * is + iy) * is + ix];
                        z = z + wc[(ci * k + ky) * k + kx] * v;
                    }
                }
            z = z + bias[co];
            out[e] = relu ? (z > 0.0f ? z : 0.0f) : z;
        }
    } else {
        // one wave per unit: lane c sums k = c (mod 64) in k order, then a fixed xor tree
        const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
        for (int j = wave; j < q.n_out; j += nw) {
            const float* wj = w + (int64_t)j * q.K;
            float s = 0.0f;
            for (int kk = lane; kk < q.K; kk += 64) s = s + wj[kk] * x[kk];
            for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m);
            const float z = s + bias[j];
            if (lane == 0) out[j] = relu ? (z > 0.0f ? z : 0.0f) : z;
        }
    }
}

// dL/dz of layer l - 1 from layer l's deltas and weights: relu'(z_{l-1}) * (W_l^T delta_l), the conv layers'
// transposed convolution as a gather per input element (an input no window covers sums nothing: exactly 0).
__device__ __forceinline__ void cl_backward(const Plan& P, int l, const float* __restrict__ W, float* row) {
    const LLayer& q = P.l[l];
    const LLayer& pv = P.l[l - 1];
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* w = W + q.woff;
    const float* d = row + q.delta;
    const float* h = row + pv.act;
    float* out = row + pv.delta;
    if (q.conv) {
        const int os = q.out_side, is = q.in_side, hw = is * is, k = q.k;
        for (int e = tid; e < q.n_in; e += nt) {
            const int ci = e / hw, pos = e - ci * hw, iy = pos / is, ix = pos - iy * is;
            float s = 0.0f;
            for (int co = 0; co < q.cout; ++co)
                for (int ky = 0; ky < k; ++ky) {
                    const int ty = iy + q.p - ky;
                    if (ty < 0 || ty % q.s) continue;
                    const int oy = ty / q.s;
                    if (oy >= os) continue;
                    for (int kx = 0; kx < k; ++kx) {
                        const int tx = ix + q.p - kx;
                        if (tx < 0 || tx % q.s) continue;
                        const int ox = tx / q.s;
                        if (ox >= os) continue;
                        s = s + d[(co * os + oy) * os + ox] * w[(((int64_t)co * q.cin + ci) * k + ky) * k + kx];
                    }
                }
            out[e] = h[e] > 0.0f ? s : 0.0f;
        }
    } else {
        for (int i = tid; i < q.n_in; i += nt) {
            float s = 0.0f;
            for (int j = 0; j < q.n_out; ++j) s = s + d[j] * w[(int64_t)j * q.K + i];
            out[i] = h[i] > 0.0f ? s : 0.0f;
        }
    }
}

}  // namespace

}  // namespace cl
}  // namespace drl
