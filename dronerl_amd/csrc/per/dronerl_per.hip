// dronerl_per.hip — prioritized experience replay on the device (Schaul et al. 2016, the proportional variant;
// include/dronerl.h drl_per_* and drl_dqn_per_train; the block's layout in dronerl_per_layout.h):
//   drl_per_init_kernel      the tree zeroed, pmax = 1;
//   drl_per_mark_kernel      the leaves of freshly added slots set to pmax;
//   drl_per_rebuild_kernel   every internal node from the leaves: a workgroup reduces a run of consecutive nodes
//                            through LDS and writes all levels of that subtree; a tree of more than one run takes
//                            a second launch of one workgroup over the runs' roots.  Node = left + right, one f32
//                            addition, whoever computes it: a rebuild is bit for bit a numpy restatement;
//   drl_per_sample_kernel    one row per stratum: a counter hash places the row's mass in its stratum, the descent
//                            reads the tree's top from LDS and the rest from L2; the importance weights and their
//                            maximum (an integer max on the positive floats' bits, in LDS) in the same workgroup;
//   drl_dqn_per_rows / forward / td / priority / backward / update / blend / counters _kernel
//                            the large-batch learner's chain (largelearn/dronerl_largelearn_chain.h: the same
//                            bodies the uniform learner's kernels run) on the drawn rows.  Only the rows and the TD
//                            bodies are new (per_rows_body, per_td_body): the drawn slot instead of dq_sample, the
//                            row's weight on its squared error and on the Q head's delta, |d| kept and the slot's
//                            leaf zeroed; the priority kernel then raises each drawn leaf to its rows' largest new
//                            priority with an integer max on the float's bits (positive floats order as unsigned
//                            integers), and pmax the same way.
// No workgroup waits for another and no float atomic is used: nothing depends on scheduling.
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
__global__ void __launch_bounds__(kThreads) drl_per_init_kernel(TreeArgs t) {
    const int64_t n = 2 * t.P, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) t.tree[i] = 0.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *t.pmax = 1.0f;
        *t.wmax = 0.0f;
    }
}

// slots [cursor, cursor + count) mod capacity (count <= capacity: the host clamps it) take the priority pmax
__global__ void __launch_bounds__(kThreads) drl_per_mark_kernel(TreeArgs t, int64_t cursor, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    t.tree[t.P + (cursor + i) % t.capacity] = *t.pmax;
}

// Workgroup g: the subtree of n leaves (a power of two <= kRun) rooted at node root0 + g, whose leaves are the
// tree's nodes [(root0 + g) * n, (root0 + g + 1) * n).  heap: the subtree in heap order (index 1 its root).
__global__ void __launch_bounds__(kRebuildThreads) drl_per_rebuild_kernel(float* __restrict__ tree, int64_t root0,
                                                                          int n) {
    __shared__ __attribute__((aligned(16))) float heap[2 * kRun];
    const int tid = threadIdx.x;
    const int64_t root = root0 + blockIdx.x;
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
// Row b of B: m = ((b + u) / B) * tree[1] with u the row's hash in [0, 1); the descent goes left when the right
// child is 0.0 or m < left, so it stays inside nodes of positive value whatever the rounding does to m.
__global__ void __launch_bounds__(kSampleThreads) drl_per_sample_kernel(TreeArgs t, SampleArgs s,
                                                                        const DqnCounters* __restrict__ ctr) {
    __shared__ __attribute__((aligned(16))) float top[kTop];
    __shared__ uint32_t wmax_bits;
    const int tid = threadIdx.x;
    const float* __restrict__ tree = t.tree;
    const int n_top = (int)(2 * t.P < kTop ? 2 * t.P : kTop);
    for (int i = tid; i < n_top; i += kSampleThreads) top[i] = tree[i];
    if (tid == 0) wmax_bits = 0u;
    __syncthreads();
    const int32_t step = ctr->step;
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
        atomicMax(&wmax_bits, __float_as_uint(w[r]));  // (LDS; the weights are positive floats)
    }
    __syncthreads();
    const float wmax = __uint_as_float(wmax_bits);
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

__global__ void __launch_bounds__(kThreads) drl_dqn_per_rows_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    per_rows_body(a.P, a, a.P.batch, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

__global__ void __launch_bounds__(ll::kTileThreads) drl_dqn_per_forward_kernel(LearnArgs args, int l) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    ll::forward_body(a.P, a, a.P.batch, l, (int)blockIdx.y, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

__global__ void __launch_bounds__(kThreads) drl_dqn_per_td_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    per_td_body(a.P, a, a.P.batch, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// 6. The priorities: row b's p = (|d| + eps)^alpha (double, rounded once; at most 2^64, which a NaN becomes too)
// into its slot's leaf, which the TD kernel zeroed: the largest over the rows that drew the slot.  pmax likewise
// (a workgroup's largest first, in LDS).
__global__ void __launch_bounds__(kThreads) drl_dqn_per_priority_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ uint32_t wg_max;
    if (threadIdx.x == 0) wg_max = 0u;
    __syncthreads();
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (b < a.P.batch) {
        float p = (float)pow((double)a.absd[b] + a.per_eps, a.alpha);
        if (!(p <= kMaxPriority)) p = kMaxPriority;
        const uint32_t bits = __float_as_uint(p);
        atomicMax(reinterpret_cast<uint32_t*>(a.leaves + a.slots[b]), bits);
        atomicMax(&wg_max, bits);
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_max) atomicMax(reinterpret_cast<uint32_t*>(a.pmax), wg_max);
}

__global__ void __launch_bounds__(ll::kTileThreads) drl_dqn_per_backward_kernel(LearnArgs args, int l) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    ll::backward_body(a.P, a, a.P.batch, l, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

__global__ void __launch_bounds__(ll::kUpdateThreads) drl_dqn_per_update_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kUpdateChunk * ll::kUpdateCols];
    __shared__ __attribute__((aligned(16))) float Ds[ll::kUpdateChunk * ll::kUpdateUnits];
    ll::update_body(a.P, a, a.P.batch, (int)blockIdx.z, (int)blockIdx.x, (int)blockIdx.y, Xs, Ds);
}

// A step without a sample: the target blend when due, over the whole set.
__global__ void __launch_bounds__(kThreads) drl_dqn_per_blend_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.P.n_params) return;
    ll::blend_body(a, i);
}

// The counters (one workgroup); the act image's status vector cleared for the pack launch that follows.
__global__ void __launch_bounds__(kThreads) drl_dqn_per_counters_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float sq[ll::kMaxBatch];
    if (threadIdx.x < 4) a.pack_status[threadIdx.x] = 0u;
    ll::counters_body(a.P, a, a.P.batch, a.trained, sq);
}

// ---- launches ------------------------------------------------------------------------------------------------
int launch_init(const TreeArgs& t, hipStream_t s) {
    int64_t g = (2 * t.P + kThreads - 1) / kThreads;
    g = g > 4096 ? 4096 : g;
    hipLaunchKernelGGL(drl_per_init_kernel, dim3((unsigned)g), dim3(kThreads), 0, s, t);
    return (int)hipGetLastError();
}

int launch_mark(const TreeArgs& t, int64_t cursor, int64_t count, hipStream_t s) {
    if (count > t.capacity) count = t.capacity;
    if (count < 1) return 0;
    hipLaunchKernelGGL(drl_per_mark_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       t, cursor, count);
    return (int)hipGetLastError();
}

int launch_rebuild(const TreeArgs& t, hipStream_t s) {
    const int64_t run = rebuild_run(t.P), groups = rebuild_groups(t.P);
    if (run > 1)
        hipLaunchKernelGGL(drl_per_rebuild_kernel, dim3((unsigned)groups), dim3(kRebuildThreads), 0, s, t.tree, groups,
                           (int)run);
    if (groups > 1)  // the top: the subtree over the runs' roots, the tree's nodes [groups, 2 * groups)
        hipLaunchKernelGGL(drl_per_rebuild_kernel, dim3(1), dim3(kRebuildThreads), 0, s, t.tree, (int64_t)1,
                           (int)groups);
    return (int)hipGetLastError();
}

int launch_sample(const TreeArgs& t, const SampleArgs& a, const void* counters, hipStream_t s) {
    hipLaunchKernelGGL(drl_per_sample_kernel, dim3(1), dim3(kSampleThreads), 0, s, t, a,
                       static_cast<const DqnCounters*>(counters));
    return (int)hipGetLastError();
}

int launch_per_train(const LearnArgs& a, const TreeArgs& t, const SampleArgs& sa, hipStream_t s) {
    const ll::Plan& P = a.P;
    const dim3 eb(kThreads);
    if (a.trained) {
        if (const int e = launch_rebuild(t, s)) return e;
        if (const int e = launch_sample(t, sa, a.ctr, s)) return e;
        const int L = P.n_layers;
        const unsigned rt = (unsigned)ll::row_tiles(P), bt = (unsigned)((P.batch + kThreads - 1) / kThreads);
        const int64_t elems = 2 * (int64_t)P.batch * P.in4;
        hipLaunchKernelGGL(drl_dqn_per_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads)), eb, 0, s, a);
        for (int l = 0; l < L; ++l)
            hipLaunchKernelGGL(drl_dqn_per_forward_kernel, dim3(rt, 2, (unsigned)ll::unit_tiles(P.out[l])),
                               dim3(ll::kTileThreads), 0, s, a, l);
        hipLaunchKernelGGL(drl_dqn_per_td_kernel, dim3(bt), eb, 0, s, a);
        hipLaunchKernelGGL(drl_dqn_per_priority_kernel, dim3(bt), eb, 0, s, a);
        for (int l = L - 1; l >= 1; --l)
            hipLaunchKernelGGL(drl_dqn_per_backward_kernel, dim3(rt, 1, (unsigned)ll::unit_tiles(P.in[l])),
                               dim3(ll::kTileThreads), 0, s, a, l);
        int kt = 0, jt = 0;  // (the widest layer's tiles; a workgroup outside its layer's returns at once)
        for (int l = 0; l < L; ++l) {
            kt = ll::update_col_tiles(P, l) > kt ? ll::update_col_tiles(P, l) : kt;
            jt = ll::update_unit_tiles(P, l) > jt ? ll::update_unit_tiles(P, l) : jt;
        }
        hipLaunchKernelGGL(drl_dqn_per_update_kernel, dim3((unsigned)kt, (unsigned)jt, (unsigned)L),
                           dim3(ll::kUpdateThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL(drl_dqn_per_blend_kernel, dim3((unsigned)((P.n_params + kThreads - 1) / kThreads)), eb, 0, s,
                           a);
    }
    hipLaunchKernelGGL(drl_dqn_per_counters_kernel, dim3(1), eb, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace per
}  // namespace drl
