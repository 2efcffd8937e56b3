// dronerl_per_chain.h — the bodies of the prioritized replay's kernels (device only), shared by the single-agent
// kernels (dronerl_per.hip) and the prioritized population's (perpop/dronerl_perpop.hip), in the manner of
// largelearn/dronerl_largelearn_chain.h: both include it, so one agent's tree, draw, weights and priorities and
// a population member's cannot drift apart on the arithmetic.  A body takes the tree's view (per::TreeArgs: one
// agent's block, or a member's block with the member's own batch), the learner's view `a` (any struct with
// ll::LearnArgs' fields and per::LearnArgs' slots, weights, absd, leaves, pmax, alpha, per_eps) and the
// workgroup's coordinates, which the calling kernel reads from its grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "../largelearn/dronerl_largelearn_chain.h"
#include "dronerl_per_layout.h"

// every product and sum rounds on its own (no FMA contraction): the order tests/_per_ref.py restates
#pragma clang fp contract(off)

namespace drl {
namespace per {

// ---- the tree ------------------------------------------------------------------------------------------------
// One workgroup of kRebuildThreads (every thread calls: barriers): the subtree of n leaves (a power of two
// <= kRun) rooted at node `root`, whose leaves are the tree's nodes [root * n, (root + 1) * n).  heap: 2 * kRun
// floats of LDS, the subtree in heap order (index 1 its root).
__device__ __forceinline__ void rebuild_body(float* __restrict__ tree, int64_t root, int n, float* heap) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += kRebuildThreads) heap[n + i] = tree[root * n + i];
    __syncthreads();
    for (int w = n >> 1; w >= 1; w >>= 1) {  // the level of w nodes: heap [w, 2w), the tree's [root * w, (root + 1) * w)
        for (int i = tid; i < w; i += kRebuildThreads) {
            const ll::ll_f2 c = *reinterpret_cast<const ll::ll_f2*>(heap + 2 * (w + i));
            const float v = c.x + c.y;
            heap[w + i] = v;
            tree[root * w + i] = v;
        }
        __syncthreads();
    }
}

// ---- the sampler -----------------------------------------------------------------------------------------------
// One workgroup of kSampleThreads (every thread calls: barriers) draws t.batch rows at learner step `step`.
// Row b of B: m = ((b + u) / B) * tree[1] with u the row's hash in [0, 1); the descent goes left when the right
// child is 0.0 or m < left, so it stays inside nodes of positive value whatever the rounding does to m.  top: kTop
// floats of LDS; wmax_bits: one LDS word.
__device__ __forceinline__ void sample_body(const TreeArgs& t, const SampleArgs& s, int32_t step, float* top,
                                            uint32_t* wmax_bits) {
    const int tid = threadIdx.x;
    const float* __restrict__ tree = t.tree;
    const int n_top = (int)(2 * t.P < kTop ? 2 * t.P : kTop);
    for (int i = tid; i < n_top; i += kSampleThreads) top[i] = tree[i];
    if (tid == 0) *wmax_bits = 0u;
    __syncthreads();
    const int B = t.batch;
    const float root = top[1];
    int64_t idx[kSampleRows];
    float m[kSampleRows];
#pragma unroll
    for (int r = 0; r < kSampleRows; ++r) {
        const int b = tid + r * kSampleThreads;
        const uint64_t h = splitmix64(s.seed ^ splitmix64(((uint64_t)(uint32_t)step << 16) | (uint64_t)b));
        const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
        m[r] = ((float)b + u) / (float)B * root;
        idx[r] = 1;
    }
    // the rows of a thread descend level by level together: their loads are independent and stay in flight
    for (int lvl = 0; lvl < t.logP; ++lvl) {
        const bool in_lds = ((int64_t)2 << lvl) < kTop;  // the children's level lies below kTop: uniform
#pragma unroll
        for (int r = 0; r < kSampleRows; ++r) {
            if (tid + r * kSampleThreads >= B) continue;
            const int64_t c = 2 * idx[r];
            const ll::ll_f2 lr = in_lds ? *reinterpret_cast<const ll::ll_f2*>(top + c)
                                        : *reinterpret_cast<const ll::ll_f2*>(tree + c);
            if (lr.y == 0.0f || m[r] < lr.x) {
                idx[r] = c;
            } else {
                m[r] = m[r] - lr.x;
                idx[r] = c + 1;
            }
        }
    }
    double beta = s.beta0;
    if (s.beta_steps > 0) {
        const double f = (double)step / (double)s.beta_steps;
        beta = s.beta0 + (1.0 - s.beta0) * (f < 1.0 ? f : 1.0);
    }
    float w[kSampleRows];
#pragma unroll
    for (int r = 0; r < kSampleRows; ++r) {
        const int b = tid + r * kSampleThreads;
        w[r] = 0.0f;
        if (b >= B) continue;
        const float leaf = tree[idx[r]];
        w[r] = (float)pow((double)s.size * ((double)leaf / (double)root), -beta);
        // (a pad leaf is 0.0 and never entered; the clamp only keeps a tree the caller filled wrongly from naming
        // a slot outside the ring)
        const int64_t slot = idx[r] - t.P;
        t.slots[b] = slot < t.capacity ? slot : t.capacity - 1;
        atomicMax(wmax_bits, __float_as_uint(w[r]));  // (LDS; the weights are positive floats)
    }
    __syncthreads();
    const float wmax = __uint_as_float(*wmax_bits);
    if (tid == 0) *t.wmax = wmax;
#pragma unroll
    for (int r = 0; r < kSampleRows; ++r) {
        const int b = tid + r * kSampleThreads;
        if (b < B) t.weights[b] = w[r] / wmax;
    }
}

// ---- the learner -----------------------------------------------------------------------------------------------
// 1. The rows: ll::rows_body with the drawn slot in place of dq_sample.
template <class A>
__device__ __forceinline__ void per_rows_body(const ll::Plan& P, const A& a, int B, int64_t e) {
    const int64_t per = (int64_t)B * P.in4;
    if (e >= 2 * per) return;
    const int n = e >= per ? 1 : 0;
    const int64_t r = e - n * per;
    const int b = (int)(r / P.in4), k = (int)(r - (int64_t)b * P.in4);
    const int64_t s = a.slots[b];
    a.scratch[ll::x_word(P, n, b, k)] = k < P.in[0] ? dq_input(a, n ? a.r_next : a.r_obs, s, k) : 0.0f;
    if (n == 0 && k == 0) {
        reinterpret_cast<int32_t*>(a.scratch)[P.act_off + b] = a.r_act[s];
        a.scratch[P.rew_off + b] = a.r_rew[s];
        a.scratch[P.done_off + b] = a.r_done[s] ? 1.0f : 0.0f;
    }
}

// 3. The TD error of row b: ll::td_body with the row's importance weight w on its squared error and on the Q
// head's delta; |d| is kept for the priority kernel and the slot's leaf zeroed, so that the integer max there
// starts from 0.0 (a slot drawn by several rows is zeroed by each of them: the same store).
template <class A>
__device__ __forceinline__ void per_td_body(const ll::Plan& P, const A& a, int B, int b) {
    if (b >= B) return;
    const int L = P.n_layers, NA = P.out[L - 1];
    const float* q = a.scratch + ll::h_word(P, 0, L - 1, b, 0);
    const float* qt = a.scratch + ll::h_word(P, 1, L - 1, b, 0);
    float mx = qt[0];
    for (int j = 1; j < NA; ++j) mx = qt[j] > mx ? qt[j] : mx;  // jnp.max
    const int act = reinterpret_cast<const int32_t*>(a.scratch)[P.act_off + b];
    const float rew = a.scratch[P.rew_off + b];
    const float notdone = a.scratch[P.done_off + b] != 0.0f ? 0.0f : 1.0f;
    const float td = rew + (a.gamma * mx) * notdone;
    const bool ok = act >= 0 && act < NA;
    float qa = td;
    for (int j = 0; j < NA; ++j)
        if (ok && j == act) qa = q[j];
    const float d = qa - td;
    const float w = a.weights[b];
    a.scratch[P.sq_off + b] = w * (d * d);
    float* dq = a.scratch + ll::d_word(P, L - 1, b, 0);
    const float g = w * ((d + d) / (float)B);
    for (int j = 0; j < P.ld[L - 1]; ++j) dq[j] = (ok && j == act) ? g : 0.0f;
    a.absd[b] = __builtin_fabsf(d);
    a.leaves[a.slots[b]] = 0.0f;
}

// 6. The priorities (a workgroup of kThreads, every thread calls: barriers): row b's p = (|d| + eps)^alpha
// (double, rounded once; at most 2^64, which a NaN becomes too) into its slot's leaf, which the TD kernel zeroed:
// the largest over the rows that drew the slot.  pmax likewise (a workgroup's largest first, in LDS: wg_max).
template <class A>
__device__ __forceinline__ void priority_body(const A& a, int B, int b, uint32_t* wg_max) {
    if (threadIdx.x == 0) *wg_max = 0u;
    __syncthreads();
    if (b < B) {
        float p = (float)pow((double)a.absd[b] + a.per_eps, a.alpha);
        if (!(p <= kMaxPriority)) p = kMaxPriority;
        const uint32_t bits = __float_as_uint(p);
        atomicMax(reinterpret_cast<uint32_t*>(a.leaves + a.slots[b]), bits);
        atomicMax(wg_max, bits);
    }
    __syncthreads();
    if (threadIdx.x == 0 && *wg_max) atomicMax(reinterpret_cast<uint32_t*>(a.pmax), *wg_max);
}

}  // namespace per
}  // namespace drl
