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
//   drl_dqn_per_rows / td / priority _kernel
//                            what the large-batch learner's chain (largelearn/) does differently on drawn rows.
//                            The rows and the TD kernels run the uniform chain's bodies (ll::rows_body,
//                            ll::td_body) with the drawn rows as the rows' policy (dronerl_learn_common.h): the
//                            drawn slot instead of dq_sample, the row's weight on its squared error and on the Q
//                            head's delta, |d| kept and the slot's leaf zeroed; the priority kernel then raises
//                            each drawn leaf to its rows' largest new priority with an integer max on the float's
//                            bits (positive floats order as unsigned integers), and pmax the same way.  The
//                            forward, backward, update, blend and counters launches of a step are the uniform
//                            learner's own kernels (ll::launch_large_*), on the base of the arguments.
// The rebuild's, the sampler's and the priority kernel's bodies live in dronerl_per_chain.h, which the prioritized
// population (perpop/dronerl_perpop.hip) includes too.
// No workgroup waits for another and no float atomic is used: nothing depends on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "../largelearn/dronerl_largelearn_chain.h"
#include "dronerl_per_layout.h"
#include "dronerl_per_chain.h"

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
    rebuild_body(tree, root0 + blockIdx.x, n, heap);
}

// ---- the sampler (sample_body, dronerl_per_chain.h) ------------------------------------------------------------
__global__ void __launch_bounds__(kSampleThreads) drl_per_sample_kernel(TreeArgs t, SampleArgs s,
                                                                        const DqnCounters* __restrict__ ctr) {
    __shared__ __attribute__((aligned(16))) float top[kTop];
    __shared__ uint32_t wmax_bits;
    sample_body(t, s, ctr->step, top, &wmax_bits);
}

// ---- the learner: the chain's rows and TD bodies on the drawn rows (a.d), and the priorities ------------------
// 1. The rows (ll::rows_body): the drawn slot in place of dq_sample.
__global__ void __launch_bounds__(kThreads) drl_dqn_per_rows_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    ll::rows_body(a.P, a, a.d, a.P.batch, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// 3. The TD error (ll::td_body): the row's weight on its squared error and on the Q head's delta, |d| kept, the
// slot's leaf zeroed.
__global__ void __launch_bounds__(kThreads) drl_dqn_per_td_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    ll::td_body(a.P, a, a.d, a.P.batch, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// The priorities (priority_body): each drawn leaf raised to its rows' largest new priority, and pmax.
__global__ void __launch_bounds__(kThreads) drl_dqn_per_priority_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ uint32_t wg_max;
    priority_body(a.d, a.P.batch, (int)(blockIdx.x * kThreads + threadIdx.x), &wg_max);
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

// ---- the chain's segments which the Double DQN chain (doubledqn/) launches as they are: the rows at the drawn
// slots, and the priorities behind a TD launch.  (No error is read: the caller reads hipGetLastError behind its
// last launch.)
void launch_per_rows(const LearnArgs& a, hipStream_t s) {
    const int64_t elems = 2 * (int64_t)a.P.batch * a.P.in4;
    hipLaunchKernelGGL(drl_dqn_per_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       a);
}

void launch_per_priority(const LearnArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_dqn_per_priority_kernel, dim3((unsigned)((a.P.batch + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, a);
}

// The uniform chain (ll::launch_large_train) on the drawn rows: rebuild and sample in front, this unit's rows and
// TD kernels in place of the uniform ones, the priorities behind the TD; every other launch is the uniform
// chain's own kernel with the uniform arguments (a's base).
int launch_per_train(const LearnArgs& a, const TreeArgs& t, const SampleArgs& sa, hipStream_t s) {
    const ll::Plan& P = a.P;
    const dim3 eb(kThreads);
    if (a.trained) {
        if (const int e = launch_rebuild(t, s)) return e;
        if (const int e = launch_sample(t, sa, a.ctr, s)) return e;
        const unsigned bt = (unsigned)((P.batch + kThreads - 1) / kThreads);
        launch_per_rows(a, s);
        ll::launch_large_forward(a, s);
        hipLaunchKernelGGL(drl_dqn_per_td_kernel, dim3(bt), eb, 0, s, a);
        launch_per_priority(a, s);
        ll::launch_large_backward_update(a, s);
    } else {
        ll::launch_large_blend(a, s);
    }
    ll::launch_large_counters(a, s);
    return (int)hipGetLastError();
}

}  // namespace per
}  // namespace drl
