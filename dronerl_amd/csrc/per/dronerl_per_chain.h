// dronerl_per_chain.h — the bodies of the prioritized replay's kernels (device only), shared by the single-agent
// kernels (dronerl_per.hip), the prioritized population's (perpop/dronerl_perpop.hip) and, for the priorities, the
// conv learner's (convper/dronerl_convper.hip), in the manner of largelearn/dronerl_largelearn_chain.h: all
// include it, so one agent's tree, draw, weights and priorities and a population member's cannot drift apart on
// the arithmetic.  A body takes the tree's view (per::TreeArgs: one agent's block, or a member's block with the
// member's own batch) or the step's drawn rows (per::Drawn) and the workgroup's coordinates, which the calling
// kernel reads from its grid.
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
// The rows and the TD error are the uniform chain's bodies (ll::rows_body, ll::td_body) with the drawn rows as
// their rows' policy (dronerl_learn_common.h).
//
// 6. The priorities (a workgroup of kThreads, every thread calls: barriers): row b's p = (|d| + eps)^alpha
// (double, rounded once; at most 2^64, which a NaN becomes too) into its slot's leaf, which the TD kernel zeroed:
// the largest over the rows that drew the slot.  pmax likewise (a workgroup's largest first, in LDS: wg_max).
__device__ __forceinline__ void priority_body(const Drawn& a, int B, int b, uint32_t* wg_max) {
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
