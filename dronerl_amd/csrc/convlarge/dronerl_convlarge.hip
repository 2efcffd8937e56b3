// dronerl_convlarge.hip — the DQN learner for conv Q-networks at replay batches up to 4096 (include/dronerl.h
// drl_convnet_dqn_large_*): one train_jax.py:68-98 learner block with network_type == 'conv', with
// drl_convnet_dqn_train's semantics, as a fixed chain of stream-ordered launches (the host API then re-packs the
// act's image with the pack kernel):
//   1. drl_convnet_dqn_large_rows_kernel, one workgroup per sampled row (256 threads; up to 1024, by the widest
//      layer, at batches up to 512: a row's arithmetic does not depend on the count): drl_convnet_dqn_rows_kernel's row (the target net
//      on next_obs, the online net on obs, the TD error, the head's deltas 2 (q - td) / B with the full batch B,
//      the backward pass to every layer's dL/dz; convlearn/dronerl_convlearn_rows.h), to the scratch;
//   2. drl_convnet_dqn_large_dense_grad_kernel: the rows are cut into chunks of 64 (chunk c: rows 64 c ..), and a
//      workgroup takes (chunk, 32 units, 64 columns of [W_l | b_l]) of a dense layer: the chunk's deltas and
//      inputs staged once in LDS, a thread keeps 8 units of one column in registers and adds the chunk's rows in
//      row order from 0.0 -- the chunk's partial gradient, to the scratch;
//   3. drl_convnet_dqn_large_conv_grad_kernel, one wave per (chunk, conv parameter group: the k x k weights of
//      one (co, ci), or one bias): each parameter's chunk terms (row, position) dealt to the lanes by
//      (b hw + pos) mod 64, each lane's in t order, then the fixed xor tree -- what
//      drl_convnet_dqn_update_kernel does for its whole batch;
//   4. drl_convnet_dqn_large_update_kernel, one thread per parameter: g = p[0] + p[1] + ... in chunk order, Adam,
//      the target blend when due (in a step without a sample: the blend alone);
//   5. drl_convnet_dqn_large_counters_kernel: the loss (each chunk's squared errors in row order, the chunk sums
//      in chunk order, / B), Adam's count and powers, the epsilon decay, step + 1 -- the only writer of the
//      counters, behind every reader in stream order; it also clears the act image's status vector for the pack
//      launch behind it.
// No workgroup waits for another and no float atomic is used: the result does not depend on scheduling.  With
// one chunk (B <= 64) every sum is drl_convnet_dqn_train's own, so the two learners agree bit for bit.  An MFMA
// sums its K products in an order of its own, so the partials are VALU work.  Every loop bound is the validated
// plan's (dronerl_convlarge_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "../convlearn/dronerl_convlearn_rows.h"
#include "dronerl_convlarge_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace cg {

using cl::LLayer;

namespace {
typedef float cg_f4 __attribute__((ext_vector_type(4)));
}

// 1. The rows: drl_convnet_dqn_rows_kernel's body on this learner's arguments (the shared per-layer code is
// cl_forward / cl_backward; the head's delta divides by the full batch).
__global__ void __launch_bounds__(kRowsThreadsMax) drl_convnet_dqn_large_rows_kernel(LearnArgs args) {
    // (the arguments read in place from the kernarg segment: indexing a by-value copy's layers at run time
    // would move it to private memory)
    (void)args;
    const cl::LearnArgs& a = ((const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr())->a;
    const cl::Plan& P = a.P;
    extern __shared__ float4 cg_lds4[];
    float* row = reinterpret_cast<float*>(cg_lds4);
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
        cl::cl_forward(P, l, a.target, row);
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
        cl::cl_forward(P, l, a.online, row);
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
        cl::cl_backward(P, l, a.online, row);
        __syncthreads();
    }
    float* dst = a.scratch + P.rows_off + (int64_t)b * P.row_words;
    for (int i = tid; i < P.row_words; i += nt) dst[i] = row[i];
}

// 2. A dense layer's chunk partials: workgroup (tile blockIdx.x, chunk blockIdx.y).  The tile is kTileUnits
// units by kTileCols columns of [W_l | b_l] -- the bias is column K, whose input is 1.0 (d * 1.0 == d exactly, so
// its sum is the sum of the deltas).  Thread (column = lane, the wave's kUnitsPerThread units) sums
// dW[j][k] = sum over the chunk's rows, in row order from 0.0, of D[b][j] * x[b][k].
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_dense_grad_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::LearnArgs& a = full.a;
    const cl::Plan& P = a.P;
    __shared__ __attribute__((aligned(16))) float Xs[kChunkRows * kTileCols];
    __shared__ __attribute__((aligned(16))) float Ds[kChunkRows * kTileUnits];
    const int c = blockIdx.y;
    if (c >= full.t.chunks || (int)blockIdx.x >= full.t.dense_tiles) return;
    const TileRef tr = tile_locate(P, full.t, blockIdx.x);
    const LLayer& q = P.l[tr.layer];
    const int K = q.K, J = q.n_out, rw = P.row_words;
    const int b0 = c * kChunkRows, rows = min(kChunkRows, P.batch - b0);
    const float* base = a.scratch + P.rows_off + (int64_t)b0 * rw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const int k = tr.k0 + lane;  // the chunk's inputs, columns [k0, k0 + 64): 1.0 in column K, 0.0 past it
        for (int r = wave; r < rows; r += kThreads / 64)
            Xs[r * kTileCols + lane] = k < K ? base[(int64_t)r * rw + q.in + k] : (k == K ? 1.0f : 0.0f);
        const int u = tid % kTileUnits, j = tr.j0 + u;  // the chunk's deltas, units [j0, j0 + 32): 0.0 past J
        for (int r = tid / kTileUnits; r < rows; r += kThreads / kTileUnits)
            Ds[r * kTileUnits + u] = j < J ? base[(int64_t)r * rw + q.delta + j] : 0.0f;
    }
    __syncthreads();
    static_assert(kUnitsPerThread == 8 && kTileCols == 64, "two 16-B reads of the wave's deltas; a lane per column");
    float g[kUnitsPerThread];
#pragma unroll
    for (int u = 0; u < kUnitsPerThread; ++u) g[u] = 0.0f;
    const float* xs = Xs + lane;
    const float* ds = Ds + wave * kUnitsPerThread;
    for (int r = 0; r < rows; ++r) {  // rows in row order
        const float x = xs[r * kTileCols];
        const cg_f4 d0 = *reinterpret_cast<const cg_f4*>(ds + r * kTileUnits);
        const cg_f4 d1 = *reinterpret_cast<const cg_f4*>(ds + r * kTileUnits + 4);
        g[0] = g[0] + d0.x * x;
        g[1] = g[1] + d0.y * x;
        g[2] = g[2] + d0.z * x;
        g[3] = g[3] + d0.w * x;
        g[4] = g[4] + d1.x * x;
        g[5] = g[5] + d1.y * x;
        g[6] = g[6] + d1.z * x;
        g[7] = g[7] + d1.w * x;
    }
    const int k = tr.k0 + lane;
    if (k > K) return;
#pragma unroll
    for (int u = 0; u < kUnitsPerThread; ++u) {
        const int j = tr.j0 + wave * kUnitsPerThread + u;
        if (j >= J) break;
        const int64_t i = k < K ? q.woff + (int64_t)j * K + k : q.boff + j;
        a.scratch[part_word(P, full.t, c, i)] = g[u];
    }
}

namespace {

// A conv parameter group's chunk partials, one wave: the KS x KS weights of (layer, co, ci), or (ci == cin) the
// bias of (layer, co).  Each parameter's sum is drl_convnet_dqn_update_kernel's over the chunk's rows: term
// t = bl * hw + pos (bl the row within the chunk: 64 c hw == 0 mod 64, so the deal is the whole batch's) goes to
// lane t mod 64, a lane adds its terms in t order (a term whose input falls outside the map adds nothing), then
// the fixed xor tree.  The group shares a term's index arithmetic and its delta among its parameters.
template <int KS>
__device__ __forceinline__ void cg_conv_group(const cl::Plan& P, const GroupRef r, const float* __restrict__ rows,
                                              int nb, float* __restrict__ part) {
    const LLayer& q = P.l[r.layer];
    const int lane = threadIdx.x & 63, rw = P.row_words;
    const int os = q.out_side, is = q.in_side, hw = os * os;
    if (r.ci == q.cin) {  // the bias
        float g = 0.0f;
        for (int t = lane; t < nb * hw; t += 64) {
            const int b = t / hw, pos = t - b * hw;
            g = g + rows[(int64_t)b * rw + q.delta + r.co * hw + pos];
        }
        for (int m = 1; m < 64; m <<= 1) g = g + __shfl_xor(g, m);
        if (lane == 0) part[q.boff + r.co] = g;
        return;
    }
    float g[KS * KS];
#pragma unroll
    for (int e = 0; e < KS * KS; ++e) g[e] = 0.0f;
    for (int t = lane; t < nb * hw; t += 64) {
        const int b = t / hw, pos = t - b * hw;
        const float d = rows[(int64_t)b * rw + q.delta + r.co * hw + pos];
        const int oy = pos / os, ox = pos - oy * os;
        const float* x = rows + (int64_t)b * rw + q.in;
        // (no branch per term: the input is read at a clamped place and the sum kept as it was when the term
        // falls outside the map, so a term's KS x KS loads are in flight together)
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const int iy = oy * q.s + ky - q.p, iyc = min(max(iy, 0), is - 1);
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const int ix = ox * q.s + kx - q.p, ixc = min(max(ix, 0), is - 1);
                const bool inside = iy >= 0 && iy < is && ix >= 0 && ix < is;
                // layer 0 reads the observation's [y][x][c]; later layers the previous [c][y][x]
                const float v = r.layer == 0 ? x[(iyc * is + ixc) * 6 + r.ci] : x[(r.ci * is + iyc) * is + ixc];
                const float sum = g[ky * KS + kx] + d * v;
                g[ky * KS + kx] = inside ? sum : g[ky * KS + kx];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < KS * KS; ++e)
        for (int m = 1; m < 64; m <<= 1) g[e] = g[e] + __shfl_xor(g[e], m);
    if (lane != 0) return;
    float* w = part + q.woff + ((int64_t)r.co * q.cin + r.ci) * (KS * KS);
#pragma unroll
    for (int e = 0; e < KS * KS; ++e) w[e] = g[e];
}

}  // namespace

// 3. The conv layers' chunk partials: wave (parameter group, chunk blockIdx.y), kConvWaves groups per workgroup.
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_conv_grad_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::LearnArgs& a = full.a;
    const cl::Plan& P = a.P;
    const int c = blockIdx.y;
    const int gi = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kConvWaves + (int)(threadIdx.x >> 6));
    if (gi >= full.t.conv_groups || c >= full.t.chunks) return;  // (the whole wave)
    const GroupRef r = group_locate(P, full.t, gi);
    const int b0 = c * kChunkRows, nb = min(kChunkRows, P.batch - b0);
    const float* rows = a.scratch + P.rows_off + (int64_t)b0 * P.row_words;
    float* part = a.scratch + part_word(P, full.t, c, 0);
    static_assert(kMaxKernel == 5, "one instantiation per kernel size");
    switch (P.l[r.layer].k) {
        case 1: cg_conv_group<1>(P, r, rows, nb, part); break;
        case 2: cg_conv_group<2>(P, r, rows, nb, part); break;
        case 3: cg_conv_group<3>(P, r, rows, nb, part); break;
        case 4: cg_conv_group<4>(P, r, rows, nb, part); break;
        default: cg_conv_group<5>(P, r, rows, nb, part); break;
    }
}

// 4. The parameters, a thread each: the chunk partials in chunk order, Adam, the target blend when due.
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_update_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::LearnArgs& a = full.a;
    const cl::Plan& P = a.P;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.n_params) return;
    const int32_t step = a.ctr->step;
    const bool due = step % a.target_every == 0;
    if (!a.trained) {  // buffer.can_sample is false: no train_step; the target blend when due
        if (due) a.target[i] = dq_blend(a, a.online[i], a.target[i]);
        return;
    }
    // Adam's bias corrections for this step (count + 1): 1 - beta^count in double, rounded once
    const float bc1 = (float)(1.0 - a.ctr->beta1_pow * a.b1d), bc2 = (float)(1.0 - a.ctr->beta2_pow * a.b2d);
    float g = a.scratch[part_word(P, full.t, 0, i)];
    for (int c = 1; c < full.t.chunks; ++c) g = g + a.scratch[part_word(P, full.t, c, i)];  // chunk order
    float m = a.adam_m[i], v = a.adam_v[i];
    const float nw = dq_adam(a, a.online[i], g, &m, &v, bc1, bc2);
    a.online[i] = nw;
    a.adam_m[i] = m;
    a.adam_v[i] = v;
    if (due) a.target[i] = dq_blend(a, nw, a.target[i]);
}

// 5. The counters (one wave): thread c sums chunk c's squared errors in row order, thread 0 the chunk sums in
// chunk order.
__global__ void __launch_bounds__(64) drl_convnet_dqn_large_counters_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::LearnArgs& a = full.a;
    __shared__ float cs[kMaxChunks];
    const int B = a.P.batch, tid = threadIdx.x;
    // the act image's status vector, cleared for the pack launch that follows (a store, not a memset: a
    // captured call then holds kernel nodes only, as the conv learner's)
    if (tid < 4) a.pack_status[tid] = 0u;
    if (a.trained && tid < full.t.chunks) {
        const int b0 = tid * kChunkRows, b1 = min(b0 + kChunkRows, B);
        float s = 0.0f;
        for (int b = b0; b < b1; ++b) s = s + a.scratch[a.P.sq_off + b];
        cs[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const DqnCounters ctr = *a.ctr;
    float loss = 0.0f, bc1 = 0.0f, bc2 = 0.0f;
    if (a.trained) {
        loss = cs[0];
        for (int c = 1; c < full.t.chunks; ++c) loss = loss + cs[c];
        loss = loss / (float)B;  // jnp.mean(jnp.square(q - td))
        bc1 = (float)(1.0 - ctr.beta1_pow * a.b1d);
        bc2 = (float)(1.0 - ctr.beta2_pow * a.b2d);
    }
    dq_finish_counters(a, a.ctr, ctr, a.trained, loss, bc1, bc2);
}

// The replay slots the next drl_convnet_dqn_large_train launch samples (its step counter as it stands on the
// stream)
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_sample_kernel(const DqnCounters* c, uint64_t seed,
                                                                                int batch, int64_t size,
                                                                                int64_t* out) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b < batch) out[b] = dq_sample(seed, c->step, b, size);
}

int launch_convlarge_train(const LearnArgs& a, hipStream_t s) {
    const cl::Plan& P = a.a.P;
    const unsigned chunks = (unsigned)a.t.chunks;
    if (a.a.trained) {
        hipLaunchKernelGGL(drl_convnet_dqn_large_rows_kernel, dim3((unsigned)P.batch),
                           dim3((unsigned)a.t.rows_threads), (size_t)P.row_words * 4, s, a);
        hipLaunchKernelGGL(drl_convnet_dqn_large_dense_grad_kernel, dim3((unsigned)a.t.dense_tiles, chunks),
                           dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(drl_convnet_dqn_large_conv_grad_kernel,
                           dim3((unsigned)((a.t.conv_groups + kConvWaves - 1) / kConvWaves), chunks), dim3(kThreads),
                           0, s, a);
    }
    hipLaunchKernelGGL(drl_convnet_dqn_large_update_kernel, dim3((unsigned)((P.n_params + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_convnet_dqn_large_counters_kernel, dim3(1), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int launch_convlarge_sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(drl_convnet_dqn_large_sample_kernel, dim3((unsigned)((batch + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, static_cast<const DqnCounters*>(counters), seed, batch, size, out);
    return (int)hipGetLastError();
}

}  // namespace cg
}  // namespace drl
