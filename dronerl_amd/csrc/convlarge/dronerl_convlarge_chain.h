// dronerl_convlarge_chain.h — the bodies of the conv large-batch learner's launch chain, shared by
// convlarge/dronerl_convlarge.hip (one agent: drl_convnet_dqn_large_*) and convpop/dronerl_convpop.hip (a
// population: drl_convpop_*), in the manner of largelearn/dronerl_largelearn_chain.h: both units' kernels run
// these, so a population member's arithmetic cannot drift from the single agent's; the prioritized learner's rows
// kernel (convper/dronerl_convper.hip) runs rows_body too, on its drawn rows.  A body takes the validated
// plan (cl::Plan and cg::Tiles: every loop bound), an agent view `a` (any struct with cl::LearnArgs' field names:
// the parameter sets, the counters, the scratch, the replay ring and the hyperparameters, which
// dronerl_learn_common.h's functions read), the batch it trains on and its workgroup coordinates.  The single
// agent passes its LearnArgs, P.batch and blockIdx; the population a member's view, that member's batch and its
// grid slice.  The scratch is laid out for the plan's batch; a smaller batch uses its first rows and chunks.
#pragma once
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

// 1. Row b of the batch (one workgroup, the row's words in LDS): drl_convnet_dqn_rows_kernel's row (the shared
// per-layer code is cl_forward / cl_backward; the head's delta divides by the full batch).  p: how the row is
// drawn and weighted (dronerl_learn_common.h: UniformRows, or the prioritized replay's drawn rows, whose weight
// lies on the squared error and on the head's delta, |d| kept and the slot's leaf zeroed for the priority kernel).
template <class V, class R>
__device__ __forceinline__ void rows_body(const cl::Plan& P, const V& a, const R& p, int batch, int b, float* row) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (b >= batch) return;
    const int L = P.n_layers, A = P.n_actions;
    const int32_t step = a.ctr->step;
    const int64_t s = dq_row_slot(p, a.seed, step, b, a.size);
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
        const auto w = dq_row_weight(p, b);
        for (int j = 0; j < A; ++j) dq[j] = (ok && j == act) ? dq_weighted(w, (d + d) / (float)batch) : 0.0f;
        a.scratch[P.sq_off + b] = dq_weighted(w, d * d);
        dq_row_keep(p, b, s, d);
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
        cl::cl_backward(P, l, a.online, row);
        __syncthreads();
    }
    float* dst = a.scratch + P.rows_off + (int64_t)b * P.row_words;
    for (int i = tid; i < P.row_words; i += nt) dst[i] = row[i];
}

// 2. A dense layer's chunk partials: workgroup (tile, chunk c) of kThreads.  The tile is kTileUnits units by
// kTileCols columns of [W_l | b_l] -- the bias is column K, whose input is 1.0 (d * 1.0 == d exactly, so its sum
// is the sum of the deltas).  Thread (column = lane, the wave's kUnitsPerThread units) sums
// dW[j][k] = sum over the chunk's rows, in row order from 0.0, of D[b][j] * x[b][k].
// Xs: kChunkRows * kTileCols floats of LDS, Ds: kChunkRows * kTileUnits, both 16-byte aligned.
template <class V>
__device__ __forceinline__ void dense_grad_body(const cl::Plan& P, const Tiles& T, const V& a, int batch, int tile,
                                                int c, float* Xs, float* Ds) {
    const TileRef tr = tile_locate(P, T, tile);
    const LLayer& q = P.l[tr.layer];
    const int K = q.K, J = q.n_out, rw = P.row_words;
    const int b0 = c * kChunkRows, rows = min(kChunkRows, batch - b0);
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
        a.scratch[part_word(P, T, c, i)] = g[u];
    }
}

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

// 3. The conv layers' chunk partials: one wave takes (parameter group gi, chunk c).
template <class V>
__device__ __forceinline__ void conv_grad_body(const cl::Plan& P, const Tiles& T, const V& a, int batch, int gi, int c) {
    const GroupRef r = group_locate(P, T, gi);
    const int b0 = c * kChunkRows, nb = min(kChunkRows, batch - b0);
    const float* rows = a.scratch + P.rows_off + (int64_t)b0 * P.row_words;
    float* part = a.scratch + part_word(P, T, c, 0);
    static_assert(kMaxKernel == 5, "one instantiation per kernel size");
    switch (P.l[r.layer].k) {
        case 1: cg_conv_group<1>(P, r, rows, nb, part); break;
        case 2: cg_conv_group<2>(P, r, rows, nb, part); break;
        case 3: cg_conv_group<3>(P, r, rows, nb, part); break;
        case 4: cg_conv_group<4>(P, r, rows, nb, part); break;
        default: cg_conv_group<5>(P, r, rows, nb, part); break;
    }
}

// 4. Parameter i (a thread): the `chunks` chunk partials in chunk order, Adam, the target blend when due; in a
// step without a sample (trained == 0: buffer.can_sample is false) the blend alone.
template <class V>
__device__ __forceinline__ void update_body(const cl::Plan& P, const Tiles& T, const V& a, int trained, int chunks,
                                            int64_t i) {
    if (i >= P.n_params) return;
    const int32_t step = a.ctr->step;
    const bool due = step % a.target_every == 0;
    if (!trained) {
        if (due) a.target[i] = dq_blend(a, a.online[i], a.target[i]);
        return;
    }
    // Adam's bias corrections for this step (count + 1): 1 - beta^count in double, rounded once
    const float bc1 = (float)(1.0 - a.ctr->beta1_pow * a.b1d), bc2 = (float)(1.0 - a.ctr->beta2_pow * a.b2d);
    float g = a.scratch[part_word(P, T, 0, i)];
    for (int c = 1; c < chunks; ++c) g = g + a.scratch[part_word(P, T, c, i)];  // chunk order
    float m = a.adam_m[i], v = a.adam_v[i];
    const float nw = dq_adam(a, a.online[i], g, &m, &v, bc1, bc2);
    a.online[i] = nw;
    a.adam_m[i] = m;
    a.adam_v[i] = v;
    if (due) a.target[i] = dq_blend(a, nw, a.target[i]);
}

// 5. The counters (one wave): thread c sums chunk c's squared errors in row order, thread 0 the chunk sums in
// chunk order.  cs: kMaxChunks floats of LDS.  pack_status (nullable): the act image's status vector, cleared
// for the pack launch that follows (a store, not a memset: a captured call then holds kernel nodes only, as the
// conv learner's); a population has no packed image.
template <class V>
__device__ __forceinline__ void counters_body(const cl::Plan& P, const V& a, int batch, int trained, int chunks,
                                              uint32_t* pack_status, float* cs) {
    const int B = batch, tid = threadIdx.x;
    if (pack_status && tid < 4) pack_status[tid] = 0u;
    if (trained && tid < chunks) {
        const int b0 = tid * kChunkRows, b1 = min(b0 + kChunkRows, B);
        float s = 0.0f;
        for (int b = b0; b < b1; ++b) s = s + a.scratch[P.sq_off + b];
        cs[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const DqnCounters ctr = *a.ctr;
    float loss = 0.0f, bc1 = 0.0f, bc2 = 0.0f;
    if (trained) {
        loss = cs[0];
        for (int c = 1; c < chunks; ++c) loss = loss + cs[c];
        loss = loss / (float)B;  // jnp.mean(jnp.square(q - td))
        bc1 = (float)(1.0 - ctr.beta1_pow * a.b1d);
        bc2 = (float)(1.0 - ctr.beta2_pow * a.b2d);
    }
    dq_finish_counters(a, a.ctr, ctr, trained, loss, bc1, bc2);
}

}  // namespace

}  // namespace cg
}  // namespace drl
