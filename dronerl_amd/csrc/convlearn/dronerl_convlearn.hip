// dronerl_convlearn.hip — the DQN learner for conv Q-networks (include/dronerl.h drl_convnet_dqn_*): one
// train_jax.py:68-98 learner block with network_type == 'conv' as three stream-ordered launches (the host API
// then re-packs the act's image):
//   1. drl_convnet_dqn_rows_kernel, one workgroup per sampled row: the row's slot (dq_sample), the target net on
//      next_obs to max_a Q, the online net on obs keeping every layer's relu(z), the TD error, 2 (q - td) / B,
//      and the backward pass to every layer's dL/dz (through the dense layers and, transposed, through the conv
//      layers >= 1), all in LDS; the row's input, activations, deltas and squared error go to the scratch;
//   2. drl_convnet_dqn_update_kernel, one thread per dense parameter and one wave per conv parameter: its
//      gradient as a sum in a fixed order (dense: rows in row order; conv: the (row, position) terms dealt to
//      the 64 lanes, each lane's in order, then a fixed xor tree), Adam, the target blend when due;
//   3. drl_convnet_dqn_counters_kernel: the loss (rows in order), Adam's count and powers, the epsilon decay,
//      step + 1 -- the only writer of the counters, behind every reader in stream order; it also clears the act
//      image's status vector for the pack launch behind it.
// No workgroup waits for another and no float atomic is used: the result does not depend on scheduling.  A batch
// of <= 64 rows of a <= 9x9 window is latency-bound f32 VALU work, not MFMA-shaped.  Activations and deltas are
// kept in torch order ([co][oy][ox]), so the flatten is the identity; relu'(z) is taken from relu(z) > 0, which
// is 0 at z == 0 as in jax and torch.  Every loop bound is the validated plan's (dronerl_convlearn_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "dronerl_convlearn_layout.h"
#include "dronerl_convlearn_rows.h"

// every product and sum rounds on its own (no FMA contraction), as in the dense learner
#pragma clang fp contract(off)

namespace drl {
namespace cl {

__global__ void __launch_bounds__(kRowsThreads) drl_convnet_dqn_rows_kernel(LearnArgs args) {
    // (the arguments read in place from the kernarg segment: indexing a by-value copy's layers at run time
    // would move it to private memory)
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    extern __shared__ float4 cl_lds4[];
    float* row = reinterpret_cast<float*>(cl_lds4);
    const int tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x;
    if (b >= P.batch) return;
    const int L = P.n_layers, A = P.n_actions;
    const int32_t step = a.ctr->step;
    const int64_t s = dq_sample(a.seed, step, b, a.size);
    for (int i = tid; i < P.row_words; i += nt) row[i] = 0.0f;
    __syncthreads();
    // the target net on next_obs: max_a Q_target
    for (int i = tid; i < P.in; i += nt) row[i] = dq_input(a, a.r_next, s, i);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        cl_forward(P, l, a.target, row);
        __syncthreads();
    }
    const float* qv = row + P.l[L - 1].delta;
    float mx = 0.0f;  // (thread 0 alone forms the TD error: it keeps the maximum in a register)
    if (tid == 0) {
        mx = qv[0];
        for (int j = 1; j < A; ++j) mx = qv[j] > mx ? qv[j] : mx;  // jnp.max
    }
    __syncthreads();
    // the online net on obs
    for (int i = tid; i < P.in; i += nt) row[i] = dq_input(a, a.r_obs, s, i);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        cl_forward(P, l, a.online, row);
        __syncthreads();
    }
    if (tid == 0) {  // the TD error and the Q head's deltas: d loss / d q[a_b] = 2 (q - td) / B
        float* dq = row + P.l[L - 1].delta;
        const int act = a.r_act[s];
        const float rew = a.r_rew[s];
        const float notdone = a.r_done[s] ? 0.0f : 1.0f;
        const float td = rew + (a.gamma * mx) * notdone;
        const bool ok = act >= 0 && act < A;  // (an action outside [0, A) adds nothing)
        const float d = (ok ? dq[act] : td) - td;
        for (int j = 0; j < A; ++j) dq[j] = (ok && j == act) ? (d + d) / (float)P.batch : 0.0f;
        a.scratch[P.sq_off + b] = d * d;
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
        cl_backward(P, l, a.online, row);
        __syncthreads();
    }
    float* dst = a.scratch + P.rows_off + (int64_t)b * P.row_words;
    for (int i = tid; i < P.row_words; i += nt) dst[i] = row[i];
}

// The update kernel's grid: the conv layers' parameters (the first of a set) take one wave each, the dense
// layers' one thread each.
__host__ __device__ inline int64_t cl_conv_params(const Plan& P) { return P.l[P.n_conv].woff; }
__host__ __device__ inline int64_t cl_conv_blocks(const Plan& P) {
    return (cl_conv_params(P) + kUpdateThreads / 64 - 1) / (kUpdateThreads / 64);
}

__global__ void __launch_bounds__(kUpdateThreads) drl_convnet_dqn_update_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    const int lane = threadIdx.x & 63;
    const int64_t nconv = cl_conv_params(P), cblocks = cl_conv_blocks(P);
    const bool wide = (int64_t)blockIdx.x < cblocks;  // a wave per parameter (uniform over the workgroup)
    const int64_t i = wide ? (int64_t)blockIdx.x * (kUpdateThreads / 64) + (threadIdx.x >> 6)
                           : nconv + ((int64_t)blockIdx.x - cblocks) * kUpdateThreads + threadIdx.x;
    if (i >= (wide ? nconv : P.n_params)) return;  // (wide: the whole wave)
    const bool writer = !wide || lane == 0;
    const int32_t step = a.ctr->step;
    const bool due = step % a.target_every == 0;
    if (!a.trained) {  // buffer.can_sample is false: no train_step; the target blend when due
        if (due && writer) a.target[i] = dq_blend(a, a.online[i], a.target[i]);
        return;
    }
    // Adam's bias corrections for this step (count + 1): 1 - beta^count in double, rounded once
    const float bc1 = (float)(1.0 - a.ctr->beta1_pow * a.b1d), bc2 = (float)(1.0 - a.ctr->beta2_pow * a.b2d);
    const ParamRef r = param_locate(P, i);
    const LLayer& q = P.l[r.layer];
    const float* rows = a.scratch + P.rows_off;
    const int B = P.batch, rw = P.row_words;
    float g = 0.0f;
    if (wide) {
        // the (row, output position) terms dealt to the lanes: lane c sums its terms t = c (mod 64) in t order
        // (rows in row order, positions in position order), then a fixed xor tree over the lanes
        const int os = q.out_side, is = q.in_side, hw = os * os;
        for (int t = lane; t < B * hw; t += 64) {
            const int b = t / hw, pos = t - b * hw;
            const float d = rows[(int64_t)b * rw + q.delta + r.co * hw + pos];
            if (r.bias) {
                g = g + d;
                continue;
            }
            const int oy = pos / os, ox = pos - oy * os;
            const int iy = oy * q.s + r.ky - q.p, ix = ox * q.s + r.kx - q.p;
            if (iy < 0 || iy >= is || ix < 0 || ix >= is) continue;
            const float* x = rows + (int64_t)b * rw + q.in;
            const float v = r.layer == 0 ? x[(iy * is + ix) * 6 + r.ci] : x[(r.ci * is + iy) * is + ix];
            g = g + d * v;
        }
        for (int m = 1; m < 64; m <<= 1) g = g + __shfl_xor(g, m);
        if (lane != 0) return;
    } else {
        for (int b = 0; b < B; ++b) {  // rows in row order
            const float d = rows[(int64_t)b * rw + q.delta + r.co];
            g = r.bias ? g + d : g + d * rows[(int64_t)b * rw + q.in + r.ci];
        }
    }
    float m = a.adam_m[i], v = a.adam_v[i];
    const float nw = dq_adam(a, a.online[i], g, &m, &v, bc1, bc2);
    a.online[i] = nw;
    a.adam_m[i] = m;
    a.adam_v[i] = v;
    if (due) a.target[i] = dq_blend(a, nw, a.target[i]);
}

__global__ void drl_convnet_dqn_counters_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    // the act image's status vector, cleared for the pack launch that follows (a store, not a memset: see the
    // host API)
    if (threadIdx.x < 4) a.pack_status[threadIdx.x] = 0u;
    if (threadIdx.x != 0) return;
    const DqnCounters ctr = *a.ctr;
    float loss = 0.0f, bc1 = 0.0f, bc2 = 0.0f;
    if (a.trained) {
        for (int b = 0; b < a.P.batch; ++b) loss = loss + a.scratch[a.P.sq_off + b];
        loss = loss / (float)a.P.batch;  // jnp.mean(jnp.square(q - td))
        bc1 = (float)(1.0 - ctr.beta1_pow * a.b1d);
        bc2 = (float)(1.0 - ctr.beta2_pow * a.b2d);
    }
    dq_finish_counters(a, a.ctr, ctr, a.trained, loss, bc1, bc2);
}

int launch_convnet_dqn_train(const LearnArgs& a, hipStream_t s) {
    if (a.trained)
        hipLaunchKernelGGL(drl_convnet_dqn_rows_kernel, dim3((unsigned)a.P.batch), dim3(kRowsThreads),
                           (size_t)a.P.row_words * 4, s, a);
    const unsigned nb = (unsigned)(cl_conv_blocks(a.P) +
                                   (a.P.n_params - cl_conv_params(a.P) + kUpdateThreads - 1) / kUpdateThreads);
    hipLaunchKernelGGL(drl_convnet_dqn_update_kernel, dim3(nb), dim3(kUpdateThreads), 0, s, a);
    hipLaunchKernelGGL(drl_convnet_dqn_counters_kernel, dim3(1), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace cl
}  // namespace drl
