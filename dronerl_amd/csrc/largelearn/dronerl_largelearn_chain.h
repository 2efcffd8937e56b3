// dronerl_largelearn_chain.h — the bodies of the large-batch learner's launch chain (device only), shared by the
// single-agent kernels (dronerl_largelearn.hip) and the population's (population/dronerl_population.hip), in the
// manner of convlearn/dronerl_convlearn_rows.h: both include it, so one agent's step and a population member's
// cannot drift apart on the arithmetic order.  The prioritized chains (per/, perpop/) run these bodies too: their
// rows and TD kernels pass the drawn rows as the rows' policy, every other step of theirs is a launch of the
// uniform kernels.  A body takes the validated plan `P` (scratch offsets, strides and
// layer sizes: sized for the block's batch), the agent's view `a` (any struct with ll::LearnArgs' pointer, replay
// and hyperparameter fields: LearnArgs itself, or a population member's view), the batch `B` the step trains on
// (P.batch for one agent; a member's own batch <= P.batch in a population) and the workgroup's coordinates, which
// the calling kernel reads from its grid.  A workgroup whose rows lie at or beyond B must not call a tile body
// (the caller returns first; the condition is uniform over the workgroup).
//
// The arithmetic order is oracle/dqn_learner.py's: a dot product keeps four partial sums over k mod 4, each in k
// order, combined (s0 + s1) + (s2 + s3), then + bias; the backward pass the same over the output index; every
// batch sum runs over the rows in order from 0.0; no product is contracted into an FMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "dronerl_largelearn_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace ll {

typedef float ll_f4 __attribute__((ext_vector_type(4)));
typedef float ll_f2 __attribute__((ext_vector_type(2)));

// out[u] = sum over k < K of A[row][k] * W[k * wk + unit(u) * wu] for this lane's row (row tile bx) and this
// wave's kUnitsPerWave units (unit tile bz), in the learner's order: partial sum c takes k = c (mod 4) in k
// order, and the four combine as (s0 + s1) + (s2 + s3).  A: rows of lda floats (lda % 4 == 0, lda >= K rounded
// up to 4; 16-B aligned).  A row past the batch and a unit past U repeat the last one (the caller stores
// neither).  Every thread of the workgroup calls it (barriers).
__device__ __forceinline__ void ll_tile(const float* __restrict__ A, int lda, int K, const float* __restrict__ W,
                                        int wk, int wu, int U, int B, int bx, int bz, float* Xs,
                                        float (&out)[kUnitsPerWave]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = bx * kTileRows;
    const int u0 = bz * kTileUnits + wave * kUnitsPerWave;
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

// 1. The rows.  Element e of 2 nets x B x in4: input k of row b's obs (n = 0) or next_obs (n = 1), 0.0 in the
// pad columns; the k = 0 element of n = 0 also gathers the row's action, reward and done.  p: how the row is
// drawn (dronerl_learn_common.h: UniformRows, or the prioritized replay's drawn rows).
template <class A, class R>
__device__ __forceinline__ void rows_body(const Plan& P, const A& a, const R& p, int B, int64_t e) {
    const int64_t per = (int64_t)B * P.in4;
    if (e >= 2 * per) return;
    const int n = e >= per ? 1 : 0;
    const int64_t r = e - n * per;
    const int b = (int)(r / P.in4), k = (int)(r - (int64_t)b * P.in4);
    const int64_t s = dq_row_slot(p, a.seed, a.ctr->step, b, a.size);
    a.scratch[x_word(P, n, b, k)] = k < P.in[0] ? dq_input(a, n ? a.r_next : a.r_obs, s, k) : 0.0f;
    if (n == 0 && k == 0) {
        reinterpret_cast<int32_t*>(a.scratch)[P.act_off + b] = a.r_act[s];
        a.scratch[P.rew_off + b] = a.r_rew[s];
        a.scratch[P.done_off + b] = a.r_done[s] ? 1.0f : 0.0f;
    }
}

// 2. Layer l of net n (0 the online net on obs, 1 the target net on next_obs), row tile bx, unit tile bz:
// z[b][j] = dot(x[b], W[j]) + bias[j]; a hidden layer stores relu(z), the Q head z.  Xs: kTileRows * kChunkStride
// floats of LDS.
// The tile itself, once the pass is chosen: parameter set `set` on the rows X (stride lda), into the rows of
// ld[l] words at scratch word `out_off`.
__device__ __forceinline__ void forward_tile(const Plan& P, int B, int l, const float* set, const float* X, int lda,
                                             float* scratch, int64_t out_off, int bx, int bz, float* Xs) {
    const int K = P.in[l], J = P.out[l];
    float z[kUnitsPerWave];
    ll_tile(X, lda, K, set + P.woff[l], 1, K, J, B, bx, bz, Xs, z);
    const int b = bx * kTileRows + (threadIdx.x & 63);
    const int j0 = bz * kTileUnits + (threadIdx.x >> 6) * kUnitsPerWave;
    if (b >= B) return;
    const float* bias = set + P.boff[l];
    float* out = scratch + (out_off + (int64_t)b * P.ld[l]);
    const bool hidden = l + 1 < P.n_layers;
#pragma unroll
    for (int u = 0; u < kUnitsPerWave; ++u) {
        const int j = j0 + u;
        if (j >= J) break;
        const float v = z[u] + bias[j];
        out[j] = hidden ? (v > 0.0f ? v : 0.0f) : v;
    }
}

template <class A>
__device__ __forceinline__ void forward_body(const Plan& P, const A& a, int B, int l, int n, int bx, int bz,
                                             float* Xs) {
    const float* set = n ? a.target : a.online;
    const float* X = a.scratch + (l == 0 ? P.x_off[n] : P.h_off[n][l - 1]);
    const int lda = l == 0 ? P.in4 : P.ld[l - 1];
    forward_tile(P, B, l, set, X, lda, a.scratch, P.h_off[n][l], bx, bz, Xs);
}

// 2b. Layer l of the Double DQN selector: the online net on next_obs, a third pass beside forward_body's two in
// the same launches.  Its activations live in the delta words d_off[l] ([batch][ld[l]], the shape of h_off[n][l]):
// nothing reads those between a step's rows launch and its TD launch, which takes the Q head's values into
// registers before it stores the deltas there; the backward launches then overwrite the layers below.
template <class A>
__device__ __forceinline__ void selector_body(const Plan& P, const A& a, int B, int l, int bx, int bz, float* Xs) {
    const float* X = a.scratch + (l == 0 ? P.x_off[1] : P.d_off[l - 1]);
    const int lda = l == 0 ? P.in4 : P.ld[l - 1];
    forward_tile(P, B, l, a.online, X, lda, a.scratch, P.d_off[l], bx, bz, Xs);
}

// 3. The TD error of row b (dqn.py:147-183): td = r + gamma * max_a Q_target * (1 - done), d = q[a] - td, the
// row's squared error and the Q head's deltas d loss / d q[b][a_b] = 2 d / B, both under the row's importance
// weight when p is a prioritized draw (dq_row_weight), which also keeps |d| and zeroes the slot's leaf
// (dq_row_keep).  An action outside [0, A) adds nothing (d = 0, no delta), as in drl_dqn_train.  T: the target
// rule (dronerl_learn_common.h).  Under DoubleTarget the next state's value is the target's at the selector's
// first maximum; the selector's Q values are the words selector_body left where the Q head's deltas go, read
// into registers before those stores.
template <class A, class R, class T = MaxTarget>
__device__ __forceinline__ void td_body(const Plan& P, const A& a, const R& p, int B, int b, const T& rule = T{}) {
    if (b >= B) return;
    const int L = P.n_layers, NA = P.out[L - 1];
    static_assert(kMaxActions <= kTargetRuleActions, "the target rule's scan covers every action");
    const float* q = a.scratch + h_word(P, 0, L - 1, b, 0);
    const float* qt = a.scratch + h_word(P, 1, L - 1, b, 0);
    float qs[kTargetRuleActions];
    dq_selector_values(rule, qs, a.scratch + d_word(P, L - 1, b, 0), NA);
    const float mx = dq_next_value(rule, qt, qs, NA);
    const int act = reinterpret_cast<const int32_t*>(a.scratch)[P.act_off + b];
    const float rew = a.scratch[P.rew_off + b];
    const float notdone = a.scratch[P.done_off + b] != 0.0f ? 0.0f : 1.0f;
    const float td = rew + (a.gamma * mx) * notdone;
    const bool ok = act >= 0 && act < NA;
    float qa = td;
    for (int j = 0; j < NA; ++j)
        if (ok && j == act) qa = q[j];
    const float d = qa - td;
    const auto w = dq_row_weight(p, b);
    a.scratch[P.sq_off + b] = dq_weighted(w, d * d);
    float* dq = a.scratch + d_word(P, L - 1, b, 0);
    const float g = dq_weighted(w, (d + d) / (float)B);
    for (int j = 0; j < P.ld[L - 1]; ++j) dq[j] = (ok && j == act) ? g : 0.0f;
    dq_row_keep(p, b, d);
}

// 4. Layer l - 1's deltas from layer l's (l >= 1): relu'(z_{l-1}) * sum over j of D_l[b][j] W_l[j][i], the
// oracle's backprop4 (the tile loop over the output index j); relu'(z) from relu(z) > 0.
template <class A>
__device__ __forceinline__ void backward_body(const Plan& P, const A& a, int B, int l, int bx, int bz, float* Xs) {
    const int J = P.out[l], I = P.in[l];
    float z[kUnitsPerWave];
    ll_tile(a.scratch + P.d_off[l], P.ld[l], J, a.online + P.woff[l], I, 1, I, B, bx, bz, Xs, z);
    const int b = bx * kTileRows + (threadIdx.x & 63);
    const int i0 = bz * kTileUnits + (threadIdx.x >> 6) * kUnitsPerWave;
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

// 5. The parameters: column tile bx, unit tile by of layer l takes kUpdateCols columns by kUpdateUnits units of
// [W_l | b_l] -- the bias is column K, whose input is 1.0 (d * 1.0 == d exactly, so its sum is the sum of the
// deltas).  Thread (column, unit pair) keeps the gradients of two units' entries in that column: dW[j][k] = sum
// over the rows, in row order, of D[b][j] * x[b][k].  A thread's chain is B dependent additions long and bounds
// the kernel, so everything else is kept off it: the rows go through LDS kUpdateChunk at a time, the next chunk's
// loads in flight while this one is summed, and a group of rows' LDS reads is issued before its sums.  (Measured:
// four units per thread lengthen each row's work, 121.6 against 92.6 us at batch 4096; two columns per thread
// 168 us.)  Then Adam, and the target blend when due.  Xs: kUpdateChunk * kUpdateCols floats of LDS, Ds:
// kUpdateChunk * kUpdateUnits.
template <class A>
__device__ __forceinline__ void update_body(const Plan& P, const A& a, int B, int l, int bx, int by, float* Xs,
                                            float* Ds) {
    const int K = P.in[l], J = P.out[l], ld = P.ld[l];
    const int k0 = bx * kUpdateCols, j0 = by * kUpdateUnits;
    if (k0 > K || j0 >= J) return;  // (the grid is the widest layer's; uniform over the workgroup)
    const int tid = threadIdx.x, kl = tid & (kUpdateCols - 1);
    const int ug = __builtin_amdgcn_readfirstlane(tid / kUpdateCols);  // the wave's unit pair
    const float* X = a.scratch + (l == 0 ? P.x_off[0] : P.h_off[0][l - 1]);
    const int lda = l == 0 ? P.in4 : P.ld[l - 1];
    const float* D = a.scratch + P.d_off[l];
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

// A step without a sample (buffer.can_sample is false): no train_step; parameter i's target blend when due.
template <class A>
__device__ __forceinline__ void blend_body(const A& a, int64_t i) {
    if (a.ctr->step % a.target_every == 0) a.target[i] = dq_blend(a, a.online[i], a.target[i]);
}

// 6. The counters (one workgroup of kThreads, every thread calls): the rows' squared errors staged in LDS (sq:
// kMaxBatch floats; a constant stride, so the loads are issued together), summed in row order by thread 0.
template <class A>
__device__ __forceinline__ void counters_body(const Plan& P, const A& a, int B, int trained, float* sq) {
    if (trained)
        for (int b = threadIdx.x; b < B; b += kThreads) sq[b] = a.scratch[P.sq_off + b];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const DqnCounters ctr = *a.ctr;
    float loss = 0.0f, bc1 = 0.0f, bc2 = 0.0f;
    if (trained) {
        for (int b = 0; b < B; ++b) loss = loss + sq[b];
        loss = loss / (float)B;  // jnp.mean(jnp.square(q - td))
        bc1 = (float)(1.0 - ctr.beta1_pow * a.b1d);
        bc2 = (float)(1.0 - ctr.beta2_pow * a.b2d);
    }
    dq_finish_counters(a, a.ctr, ctr, trained, loss, bc1, bc2);
}

}  // namespace ll
}  // namespace drl
