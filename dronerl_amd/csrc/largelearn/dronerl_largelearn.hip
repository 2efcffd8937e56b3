// dronerl_largelearn.hip — the DQN learner for dense Q-networks at replay batches up to 4096
// (include/dronerl.h drl_dqn_large_*): one train_jax.py:68-98 learner block, with drl_dqn_train's semantics and
// its arithmetic bit for bit, as a fixed chain of stream-ordered launches (the host API then re-packs the act's
// image with the pack kernel):
//   1. drl_dqn_large_rows_kernel: the rows' slots (dq_sample at the device step), their obs and next_obs decoded
//      to f32 (dq_input), their action, reward and done;
//   2. drl_dqn_large_forward_kernel, once per layer: the online net on obs and the target net on next_obs;
//   3. drl_dqn_large_td_kernel, a thread per row: max_a Q_target, the TD value, (q - td)^2 and the Q head's deltas
//      2 (q - td) / B;
//   4. drl_dqn_large_backward_kernel, once per layer >= 1: dL/dz of the layer below, masked by relu(z) > 0;
//   5. drl_dqn_large_update_kernel: each parameter's gradient as a sum over the rows in row order (the rows staged
//      through LDS in chunks), Adam, the target blend when due (drl_dqn_large_blend_kernel alone in a step without
//      a sample);
//   6. drl_dqn_large_counters_kernel: the loss (rows in order), Adam's count and powers, the epsilon decay,
//      step + 1 -- the only writer of the counters, behind every reader in stream order; it also clears the act
//      image's status vector for the pack launch behind it.
// No workgroup waits for another and no float atomic is used: the result does not depend on scheduling.
//
// The arithmetic order is oracle/dqn_learner.py's: a dot product keeps four partial sums over k mod 4, each in k
// order, combined (s0 + s1) + (s2 + s3), then + bias; the backward pass the same over the output index; every
// batch sum runs over the rows in order from 0.0; no product is contracted into an FMA.  An MFMA sums its K
// products in an order of its own, so this is VALU work.  The two matrix kernels share one tile loop (ll_tile):
// a workgroup takes 64 rows, one per lane, by 16 outputs, four per wave; the rows' operand goes through LDS in
// 128-column chunks (one 16-B read feeds the four partial sums of four outputs) and the weights are read at
// wave-uniform addresses.  Every loop bound is the validated plan's (dronerl_largelearn_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "dronerl_largelearn_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace ll {

namespace {

typedef float ll_f4 __attribute__((ext_vector_type(4)));

// out[u] = sum over k < K of A[row][k] * W[k * wk + unit(u) * wu] for this lane's row (blockIdx.x's tile) and
// this wave's kUnitsPerWave units (blockIdx.z's tile), in the learner's order: partial sum c takes k = c
// (mod 4) in k order, and the four combine as (s0 + s1) + (s2 + s3).  A: rows of lda floats (lda % 4 == 0,
// lda >= K rounded up to 4; 16-B aligned).  A row past the batch and a unit past U repeat the last one (the
// caller stores neither).  Every thread of the workgroup calls it (barriers).
__device__ __forceinline__ void ll_tile(const float* __restrict__ A, int lda, int K, const float* __restrict__ W,
                                        int wk, int wu, int U, int B, float* Xs, float (&out)[kUnitsPerWave]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * kTileRows;
    const int u0 = blockIdx.z * kTileUnits + wave * kUnitsPerWave;
    int uo[kUnitsPerWave];
#pragma unroll
    for (int u = 0; u < kUnitsPerWave; ++u) uo[u] = min(u0 + u, U - 1) * wu;
    float s[4][kUnitsPerWave];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int u = 0; u < kUnitsPerWave; ++u) s[c][u] = 0.0f;
    for (int kc = 0; kc < K; kc += kChunk) {
        const int kn = min(kChunk, K - kc), kn4 = (kn + 3) >> 2;
        __syncthreads();  // (the previous chunk's readers)
        for (int e = tid; e < kTileRows * kn4; e += kTileThreads) {
            const int r = e / kn4, q = e - r * kn4;
            const int b = min(row0 + r, B - 1);
            *reinterpret_cast<ll_f4*>(Xs + r * kChunkStride + 4 * q) =
                *reinterpret_cast<const ll_f4*>(A + (int64_t)b * lda + kc + 4 * q);
        }
        __syncthreads();
        const float* xr = Xs + lane * kChunkStride;
        const int full = kn >> 2;
        for (int q = 0; q < full; ++q) {
            const ll_f4 x = *reinterpret_cast<const ll_f4*>(xr + 4 * q);
            const float* w = W + (int64_t)(kc + 4 * q) * wk;
#pragma unroll
            for (int u = 0; u < kUnitsPerWave; ++u) {
                s[0][u] = s[0][u] + x.x * w[uo[u]];
                s[1][u] = s[1][u] + x.y * w[wk + uo[u]];
                s[2][u] = s[2][u] + x.z * w[2 * wk + uo[u]];
                s[3][u] = s[3][u] + x.w * w[3 * wk + uo[u]];
            }
        }
        const int t = kn & 3;  // (the last chunk alone: kChunk % 4 == 0)
        if (t) {
            const ll_f4 x = *reinterpret_cast<const ll_f4*>(xr + 4 * full);
            const float* w = W + (int64_t)(kc + 4 * full) * wk;
#pragma unroll
            for (int u = 0; u < kUnitsPerWave; ++u) {
                s[0][u] = s[0][u] + x.x * w[uo[u]];
                if (t > 1) s[1][u] = s[1][u] + x.y * w[wk + uo[u]];
                if (t > 2) s[2][u] = s[2][u] + x.z * w[2 * wk + uo[u]];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kUnitsPerWave; ++u) out[u] = (s[0][u] + s[1][u]) + (s[2][u] + s[3][u]);
}

}  // namespace

// 1. The rows: grid over 2 nets x batch x in4 elements.  Element (n, b, k): input k of row b's obs (n = 0) or
// next_obs (n = 1), 0.0 in the pad columns; the k = 0 thread of n = 0 also gathers the row's action, reward, done.
__global__ void __launch_bounds__(kThreads) drl_dqn_large_rows_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    const int64_t per = (int64_t)P.batch * P.in4;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= 2 * per) return;
    const int n = e >= per ? 1 : 0;
    const int64_t r = e - n * per;
    const int b = (int)(r / P.in4), k = (int)(r - (int64_t)b * P.in4);
    const int64_t s = dq_sample(a.seed, a.ctr->step, b, a.size);
    a.scratch[x_word(P, n, b, k)] = k < P.in[0] ? dq_input(a, n ? a.r_next : a.r_obs, s, k) : 0.0f;
    if (n == 0 && k == 0) {
        reinterpret_cast<int32_t*>(a.scratch)[P.act_off + b] = a.r_act[s];
        a.scratch[P.rew_off + b] = a.r_rew[s];
        a.scratch[P.done_off + b] = a.r_done[s] ? 1.0f : 0.0f;
    }
}

// 2. Layer l of both nets (blockIdx.y: 0 the online net on obs, 1 the target net on next_obs):
// z[b][j] = dot(x[b], W[j]) + bias[j]; a hidden layer stores relu(z), the Q head z.
__global__ void __launch_bounds__(kTileThreads) drl_dqn_large_forward_kernel(LearnArgs args, int l) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    __shared__ __attribute__((aligned(16))) float Xs[kTileRows * kChunkStride];
    const int n = blockIdx.y, K = P.in[l], J = P.out[l], B = P.batch;
    const float* set = n ? a.target : a.online;
    const float* A = a.scratch + (l == 0 ? P.x_off[n] : P.h_off[n][l - 1]);
    const int lda = l == 0 ? P.in4 : P.ld[l - 1];
    float z[kUnitsPerWave];
    ll_tile(A, lda, K, set + P.woff[l], 1, K, J, B, Xs, z);
    const int b = blockIdx.x * kTileRows + (threadIdx.x & 63);
    const int j0 = blockIdx.z * kTileUnits + (threadIdx.x >> 6) * kUnitsPerWave;
    if (b >= B) return;
    const float* bias = set + P.boff[l];
    float* out = a.scratch + h_word(P, n, l, b, 0);
    const bool hidden = l + 1 < P.n_layers;
#pragma unroll
    for (int u = 0; u < kUnitsPerWave; ++u) {
        const int j = j0 + u;
        if (j >= J) break;
        const float v = z[u] + bias[j];
        out[j] = hidden ? (v > 0.0f ? v : 0.0f) : v;
    }
}

// 3. The TD error of row b (dqn.py:147-183): td = r + gamma * max_a Q_target * (1 - done), d = q[a] - td, the
// row's squared error and the Q head's deltas d loss / d q[b][a_b] = 2 d / B.  An action outside [0, A) adds
// nothing (d = 0, no delta), as in drl_dqn_train.
__global__ void __launch_bounds__(kThreads) drl_dqn_large_td_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= P.batch) return;
    const int L = P.n_layers, A = P.out[L - 1];
    const float* q = a.scratch + h_word(P, 0, L - 1, b, 0);
    const float* qt = a.scratch + h_word(P, 1, L - 1, b, 0);
    float mx = qt[0];
    for (int j = 1; j < A; ++j) mx = qt[j] > mx ? qt[j] : mx;  // jnp.max
    const int act = reinterpret_cast<const int32_t*>(a.scratch)[P.act_off + b];
    const float rew = a.scratch[P.rew_off + b];
    const float notdone = a.scratch[P.done_off + b] != 0.0f ? 0.0f : 1.0f;
    const float td = rew + (a.gamma * mx) * notdone;
    const bool ok = act >= 0 && act < A;
    float qa = td;
    for (int j = 0; j < A; ++j)
        if (ok && j == act) qa = q[j];
    const float d = qa - td;
    a.scratch[P.sq_off + b] = d * d;
    float* dq = a.scratch + d_word(P, L - 1, b, 0);
    const float g = (d + d) / (float)P.batch;
    for (int j = 0; j < P.ld[L - 1]; ++j) dq[j] = (ok && j == act) ? g : 0.0f;
}

// 4. Layer l - 1's deltas from layer l's (l >= 1): relu'(z_{l-1}) * sum over j of D_l[b][j] W_l[j][i], the
// oracle's backprop4 (the tile loop over the output index j); relu'(z) from relu(z) > 0.
__global__ void __launch_bounds__(kTileThreads) drl_dqn_large_backward_kernel(LearnArgs args, int l) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    __shared__ __attribute__((aligned(16))) float Xs[kTileRows * kChunkStride];
    const int J = P.out[l], I = P.in[l], B = P.batch;
    float z[kUnitsPerWave];
    ll_tile(a.scratch + P.d_off[l], P.ld[l], J, a.online + P.woff[l], I, 1, I, B, Xs, z);
    const int b = blockIdx.x * kTileRows + (threadIdx.x & 63);
    const int i0 = blockIdx.z * kTileUnits + (threadIdx.x >> 6) * kUnitsPerWave;
    if (b >= B) return;
    const float* h = a.scratch + h_word(P, 0, l - 1, b, 0);
    float* out = a.scratch + d_word(P, l - 1, b, 0);
#pragma unroll
    for (int u = 0; u < kUnitsPerWave; ++u) {
        const int i = i0 + u;
        if (i >= I) break;
        out[i] = h[i] > 0.0f ? z[u] : 0.0f;
    }
}

// 5. The parameters: workgroup (blockIdx.x, blockIdx.y) of layer blockIdx.z takes kUpdateCols columns by
// kUpdateUnits units of [W_l | b_l] -- the bias is column K, whose input is 1.0 (d * 1.0 == d exactly, so its sum
// is the sum of the deltas).  Thread (column, unit pair) keeps the gradients of two units' entries in that
// column: dW[j][k] = sum over the rows, in row order, of D[b][j] * x[b][k].  A thread's chain is B dependent
// additions long and bounds the kernel, so everything else is kept off it: the rows go through LDS kUpdateChunk
// at a time, the next chunk's loads in flight while this one is summed, and a group of rows' LDS reads is issued
// before its sums.  (Measured: four units per thread lengthen each row's work, 121.6 against 92.6 us at batch
// 4096; two columns per thread 168 us.)  Then Adam, and the target blend when due.
__global__ void __launch_bounds__(kUpdateThreads) drl_dqn_large_update_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Plan& P = a.P;
    __shared__ __attribute__((aligned(16))) float Xs[kUpdateChunk * kUpdateCols];
    __shared__ __attribute__((aligned(16))) float Ds[kUpdateChunk * kUpdateUnits];
    const int l = blockIdx.z, B = P.batch, K = P.in[l], J = P.out[l], ld = P.ld[l];
    const int k0 = blockIdx.x * kUpdateCols, j0 = blockIdx.y * kUpdateUnits;
    if (k0 > K || j0 >= J) return;  // (the grid is the widest layer's; uniform over the workgroup)
    const int tid = threadIdx.x, kl = tid & (kUpdateCols - 1);
    const int ug = __builtin_amdgcn_readfirstlane(tid / kUpdateCols);  // the wave's unit pair
    const float* X = a.scratch + (l == 0 ? P.x_off[0] : P.h_off[0][l - 1]);
    const int lda = l == 0 ? P.in4 : P.ld[l - 1];
    const float* D = a.scratch + P.d_off[l];
    typedef float ll_f2 __attribute__((ext_vector_type(2)));
    static_assert(kUpdateThreads == kUpdateCols * (kUpdateUnits / 2) && kUpdateUnits % 4 == 0 &&
                  kUpdateChunk * (kUpdateUnits / 4) <= kUpdateThreads,
                  "a thread per (column, unit pair); at most one 16-B group of a chunk's deltas per thread");
    static_assert(kUpdateCols == 64, "a wave's lanes are one unit group's columns (ug is wave-uniform)");
    constexpr int kUpdateGroup = 16;  // rows whose LDS reads are issued together
    constexpr int XG = kUpdateChunk * (kUpdateCols / 4) / kUpdateThreads;  // 16-B groups of a chunk's inputs per thread
    ll_f4 xr[XG], dr;
    // a chunk's loads: the inputs' columns [k0, k0 + kUpdateCols) and the deltas' units [j0, j0 + kUpdateUnits),
    // 0.0 past the row stride; a row past the batch repeats the last one (never summed).  Nothing here reads a
    // loaded value, so the loads stay in flight while the chunk before is summed.
    auto load = [&](int c) {
#pragma unroll
        for (int i = 0; i < XG; ++i) {
            const int e = tid + i * kUpdateThreads, r = e / (kUpdateCols / 4), col = k0 + 4 * (e % (kUpdateCols / 4));
            const int b = min(c * kUpdateChunk + r, B - 1);
            xr[i] = ll_f4{0.0f, 0.0f, 0.0f, 0.0f};
            if (col < lda) xr[i] = *reinterpret_cast<const ll_f4*>(X + (int64_t)b * lda + col);
        }
        const int r = tid / (kUpdateUnits / 4), j = j0 + 4 * (tid % (kUpdateUnits / 4));
        const int b = min(c * kUpdateChunk + r, B - 1);
        dr = ll_f4{0.0f, 0.0f, 0.0f, 0.0f};
        if (r < kUpdateChunk && j < ld) dr = *reinterpret_cast<const ll_f4*>(D + (int64_t)b * ld + j);
    };
    // ... and their LDS stores, with column K (the bias's input) set to 1.0
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < XG; ++i) {
            const int e = tid + i * kUpdateThreads, col = k0 + 4 * (e % (kUpdateCols / 4));
            ll_f4 v = xr[i];
            if (col == K) v.x = 1.0f;
            if (col + 1 == K) v.y = 1.0f;
            if (col + 2 == K) v.z = 1.0f;
            if (col + 3 == K) v.w = 1.0f;
            *reinterpret_cast<ll_f4*>(Xs + 4 * e) = v;
        }
        if (tid < kUpdateChunk * (kUpdateUnits / 4)) *reinterpret_cast<ll_f4*>(Ds + 4 * tid) = dr;
    };
    float g[2] = {0.0f, 0.0f};
    const int chunks = (B + kUpdateChunk - 1) / kUpdateChunk;
    load(0);
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();  // (the previous chunk's readers)
        store();
        __syncthreads();
        if (c + 1 < chunks) load(c + 1);
        const int rows = min(kUpdateChunk, B - c * kUpdateChunk);
        const float* xs = Xs + kl;
        const float* ds = Ds + 2 * ug;
        int r = 0;
        for (; r + kUpdateGroup <= rows; r += kUpdateGroup) {  // rows in row order: a group's LDS reads, then its sums
            float x[kUpdateGroup];
            ll_f2 d[kUpdateGroup];
#pragma unroll
            for (int i = 0; i < kUpdateGroup; ++i) {
                x[i] = xs[(r + i) * kUpdateCols];
                d[i] = *reinterpret_cast<const ll_f2*>(ds + (r + i) * kUpdateUnits);
            }
#pragma unroll
            for (int i = 0; i < kUpdateGroup; ++i) {
                g[0] = g[0] + d[i].x * x[i];
                g[1] = g[1] + d[i].y * x[i];
            }
        }
        for (; r < rows; ++r) {
            const float x = xs[r * kUpdateCols];
            const ll_f2 d = *reinterpret_cast<const ll_f2*>(ds + r * kUpdateUnits);
            g[0] = g[0] + d.x * x;
            g[1] = g[1] + d.y * x;
        }
    }
    const int32_t step = a.ctr->step;
    const bool due = step % a.target_every == 0;
    // Adam's bias corrections for this step (count + 1): 1 - beta^count in double, rounded once
    const float bc1 = (float)(1.0 - a.ctr->beta1_pow * a.b1d), bc2 = (float)(1.0 - a.ctr->beta2_pow * a.b2d);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t i = update_param(P, l, j0 + 2 * ug + u, k0 + kl);
        if (i < 0) continue;
        float m = a.adam_m[i], v = a.adam_v[i];
        const float nwv = dq_adam(a, a.online[i], g[u], &m, &v, bc1, bc2);
        a.online[i] = nwv;
        a.adam_m[i] = m;
        a.adam_v[i] = v;
        if (due) a.target[i] = dq_blend(a, nwv, a.target[i]);
    }
}

// A step without a sample (buffer.can_sample is false): no train_step; the target blend when due, over the
// whole set as drl_dqn_train does it.
__global__ void __launch_bounds__(kThreads) drl_dqn_large_blend_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.P.n_params) return;
    if (a.ctr->step % a.target_every == 0) a.target[i] = dq_blend(a, a.online[i], a.target[i]);
}

// 6. The counters (one workgroup): the rows' squared errors staged in LDS, summed in row order by one thread.
__global__ void __launch_bounds__(kThreads) drl_dqn_large_counters_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float sq[kMaxBatch];
    const int B = a.P.batch;
    // the act image's status vector, cleared for the pack launch that follows (a store, not a memset: a
    // captured call then holds kernel nodes only, as the conv learner's)
    if (threadIdx.x < 4) a.pack_status[threadIdx.x] = 0u;
    if (a.trained)
        for (int b = threadIdx.x; b < B; b += kThreads) sq[b] = a.scratch[a.P.sq_off + b];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const DqnCounters ctr = *a.ctr;
    float loss = 0.0f, bc1 = 0.0f, bc2 = 0.0f;
    if (a.trained) {
        for (int b = 0; b < B; ++b) loss = loss + sq[b];
        loss = loss / (float)B;  // jnp.mean(jnp.square(q - td))
        bc1 = (float)(1.0 - ctr.beta1_pow * a.b1d);
        bc2 = (float)(1.0 - ctr.beta2_pow * a.b2d);
    }
    dq_finish_counters(a, a.ctr, ctr, a.trained, loss, bc1, bc2);
}

// The replay slots the next drl_dqn_large_train launch samples (its step counter as it stands on the stream)
__global__ void __launch_bounds__(kThreads) drl_dqn_large_sample_kernel(const DqnCounters* c, uint64_t seed,
                                                                        int batch, int64_t size, int64_t* out) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b < batch) out[b] = dq_sample(seed, c->step, b, size);
}

int launch_large_train(const LearnArgs& a, hipStream_t s) {
    const Plan& P = a.P;
    const dim3 eb(kThreads);
    if (a.trained) {
        const int L = P.n_layers;
        const unsigned rt = (unsigned)row_tiles(P);
        const int64_t elems = 2 * (int64_t)P.batch * P.in4;
        hipLaunchKernelGGL(drl_dqn_large_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads)), eb, 0, s, a);
        for (int l = 0; l < L; ++l)
            hipLaunchKernelGGL(drl_dqn_large_forward_kernel, dim3(rt, 2, (unsigned)unit_tiles(P.out[l])),
                               dim3(kTileThreads), 0, s, a, l);
        hipLaunchKernelGGL(drl_dqn_large_td_kernel, dim3((unsigned)((P.batch + kThreads - 1) / kThreads)), eb, 0, s, a);
        for (int l = L - 1; l >= 1; --l)
            hipLaunchKernelGGL(drl_dqn_large_backward_kernel, dim3(rt, 1, (unsigned)unit_tiles(P.in[l])),
                               dim3(kTileThreads), 0, s, a, l);
        int kt = 0, jt = 0;  // (the widest layer's tiles; a workgroup outside its layer's returns at once)
        for (int l = 0; l < L; ++l) {
            kt = update_col_tiles(P, l) > kt ? update_col_tiles(P, l) : kt;
            jt = update_unit_tiles(P, l) > jt ? update_unit_tiles(P, l) : jt;
        }
        hipLaunchKernelGGL(drl_dqn_large_update_kernel, dim3((unsigned)kt, (unsigned)jt, (unsigned)L),
                           dim3(kUpdateThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL(drl_dqn_large_blend_kernel, dim3((unsigned)((P.n_params + kThreads - 1) / kThreads)), eb, 0,
                           s, a);
    }
    hipLaunchKernelGGL(drl_dqn_large_counters_kernel, dim3(1), eb, 0, s, a);
    return (int)hipGetLastError();
}

int launch_large_sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(drl_dqn_large_sample_kernel, dim3((unsigned)((batch + kThreads - 1) / kThreads)), dim3(kThreads),
                       0, s, static_cast<const DqnCounters*>(counters), seed, batch, size, out);
    return (int)hipGetLastError();
}

}  // namespace ll
}  // namespace drl
