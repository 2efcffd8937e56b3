// dronerl_perpop.hip — prioritized replay for a population of dense DQN agents (include/dronerl.h drl_pop_per_*;
// the layout in dronerl_perpop_layout.h): every member owns a priority tree over its ring and its own (alpha,
// beta0, beta_steps, eps); the members sample, train and write their priorities back in the same launches.  The
// member is one more grid dimension, so a step's launch count does not depend on the population's size:
//   drl_pop_per_init_kernel      every member's tree zeroed, pmax = 1;
//   drl_pop_per_mark_kernel      the leaves of freshly added slots set to the member's own pmax;
//   drl_pop_per_rebuild_kernel   per::rebuild_body (a run of consecutive nodes through LDS, all levels of that
//                                subtree written) with the member in gridDim.y; a tree of more than one run takes
//                                a second launch of one workgroup per member over the runs' roots;
//   drl_pop_per_sample_kernel    per::sample_body, one workgroup per member: strata over the member's own batch,
//                                its sample_seed, its own counter's step, beta from its record;
//   drl_pop_per_rows / td / priority _kernel
//                                what the population's chain (population/dronerl_population.hip) does differently
//                                on drawn rows, a member per grid slice: the chain's rows and TD bodies
//                                (largelearn/dronerl_largelearn_chain.h) with the member's drawn rows as the rows'
//                                policy, and per::priority_body -- as drl_dqn_per_train's kernels run them.  The
//                                forward, backward, update and counters launches of a step are the population's
//                                own kernels (pop::launch_pop_*) with the population's arguments; a member's view
//                                is the population's (population/dronerl_population_member.h).
// A member trains iff size >= its batch, decided on the device from its hyperparameter record, as in
// population/dronerl_population.hip; every workgroup of a member that does not train returns at once in rebuild,
// sample, rows, forward, TD, priority and backward (its tree, pmax, slots and weights are left alone); it still
// blends its target when due, decays epsilon and advances its step.
// No workgroup waits for another, no float atomic is used (the priorities' integer max on the floats' bits is
// per/dronerl_per.hip's), nothing reads host hyperparameters: a step is graph-capturable.  Every loop bound comes
// from the validated plans.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "../largelearn/dronerl_largelearn_chain.h"
#include "../per/dronerl_per_chain.h"
#include "../population/dronerl_population_member.h"
#include "dronerl_perpop_layout.h"

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {
namespace perpop {

namespace {

using pop::hrec;

__device__ __forceinline__ const PRec& prec(const TreeSetArgs& t, int m) {
    return *reinterpret_cast<const PRec*>(t.base + t.hp_off + kPRecStride * m);
}

// member m's tree, laid out for max_batch; `batch`: the rows the member draws
__device__ __forceinline__ per::TreeArgs tree_of(const TreeSetArgs& t, int m, int batch) {
    per::TreeArgs v = per::tree_args(t.T, t.base + t.stride * m);
    v.batch = batch;
    return v;
}

// does member m take part (no gate: every member does)
__device__ __forceinline__ bool takes_part(const TreeSetArgs& t, int m) {
    return !t.gate || t.size >= hrec(t.pop, t.pop_hp_off, m).batch;
}

// member m's drawn rows, from its tree and its record: what the prioritized bodies take beside the member's view
// (pop::member_of, population/dronerl_population_member.h)
__device__ __forceinline__ per::Drawn drawn_of(const TreeSetArgs& t, int m, int batch) {
    const PRec& pr = prec(t, m);
    return per::drawn_of(tree_of(t, m, batch), pr.alpha, pr.eps);
}

}  // namespace

// ---- the trees -------------------------------------------------------------------------------------------------
// grid (tiles of the 2P nodes, members)
__global__ void __launch_bounds__(kThreads) drl_pop_per_init_kernel(TreeSetArgs t) {
    const per::TreeArgs v = tree_of(t, blockIdx.y, 0);
    const int64_t n = 2 * v.P, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) v.tree[i] = 0.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *v.pmax = 1.0f;
        *v.wmax = 0.0f;
    }
}

// grid (ceil(count / kThreads), members): slots [cursor, cursor + count) mod capacity (count <= capacity: the host
// clamps it) of every member take that member's own pmax
__global__ void __launch_bounds__(kThreads) drl_pop_per_mark_kernel(TreeSetArgs t, int64_t cursor, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const per::TreeArgs v = tree_of(t, blockIdx.y, 0);
    v.tree[v.P + (cursor + i) % v.capacity] = *v.pmax;
}

// grid (groups, members): workgroup (g, m) the subtree of n leaves rooted at node root0 + g of member m's tree
__global__ void __launch_bounds__(per::kRebuildThreads) drl_pop_per_rebuild_kernel(TreeSetArgs t, int64_t root0, int n) {
    __shared__ __attribute__((aligned(16))) float heap[2 * per::kRun];
    const int m = blockIdx.y;
    if (!takes_part(t, m)) return;  // (uniform over the workgroup)
    per::rebuild_body(reinterpret_cast<float*>(t.base + t.stride * m + t.T.pub.tree_off), root0 + blockIdx.x, n, heap);
}

// grid (members): one workgroup draws member m's rows
__global__ void __launch_bounds__(per::kSampleThreads) drl_pop_per_sample_kernel(TreeSetArgs t) {
    __shared__ __attribute__((aligned(16))) float top[per::kTop];
    __shared__ uint32_t wmax_bits;
    const int m = blockIdx.x;
    const pop::HRec& h = hrec(t.pop, t.pop_hp_off, m);
    if (t.size < h.batch) return;  // (uniform over the workgroup)
    const PRec& pr = prec(t, m);
    const per::SampleArgs s = {h.seed, t.size, pr.beta0, pr.beta_steps};
    const DqnCounters* ctr = reinterpret_cast<const DqnCounters*>(t.pop + t.pop_stride * m + t.pop_counters_off);
    per::sample_body(tree_of(t, m, h.batch), s, ctr->step, top, &wmax_bits);
}

// ---- the learner: what the population's chain does differently on drawn rows, the member in the grid ----------
// 1. rows: grid (elements of 2 x max_batch x in4, members)
__global__ void __launch_bounds__(kThreads) drl_pop_per_rows_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const pop::Member v = pop::member_of(a.p, blockIdx.y);
    if (a.p.size < v.batch) return;
    ll::rows_body(a.p.P, v, drawn_of(a.t, blockIdx.y, v.batch), v.batch, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// 3. TD: grid (max_batch rows, members); the head's deltas divide by the member's batch
__global__ void __launch_bounds__(kThreads) drl_pop_per_td_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const pop::Member v = pop::member_of(a.p, blockIdx.y);
    if (a.p.size < v.batch) return;
    ll::td_body(a.p.P, v, drawn_of(a.t, blockIdx.y, v.batch), v.batch, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// 4. the priorities: grid (max_batch rows, members), into the member's leaves and its pmax
__global__ void __launch_bounds__(kThreads) drl_pop_per_priority_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ uint32_t wg_max;
    const int batch = hrec(a.p.base, a.p.hp_off, blockIdx.y).batch;
    if (a.p.size < batch || (int)(blockIdx.x * kThreads) >= batch) return;  // (uniform over the workgroup)
    per::priority_body(drawn_of(a.t, blockIdx.y, batch), batch, (int)(blockIdx.x * kThreads + threadIdx.x), &wg_max);
}

// ---- launches ------------------------------------------------------------------------------------------------
int launch_init(const TreeSetArgs& t, hipStream_t s) {
    int64_t g = (2 * t.T.P + kThreads - 1) / kThreads;
    g = g > 4096 ? 4096 : g;
    hipLaunchKernelGGL(drl_pop_per_init_kernel, dim3((unsigned)g, (unsigned)t.members), dim3(kThreads), 0, s, t);
    return (int)hipGetLastError();
}

int launch_mark(const TreeSetArgs& t, int64_t cursor, int64_t count, hipStream_t s) {
    if (count > t.T.capacity) count = t.T.capacity;
    if (count < 1) return 0;
    hipLaunchKernelGGL(drl_pop_per_mark_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads), (unsigned)t.members),
                       dim3(kThreads), 0, s, t, cursor, count);
    return (int)hipGetLastError();
}

int launch_rebuild(const TreeSetArgs& t, hipStream_t s) {
    const int64_t run = per::rebuild_run(t.T.P), groups = per::rebuild_groups(t.T.P);
    const unsigned M = (unsigned)t.members;
    if (run > 1)
        hipLaunchKernelGGL(drl_pop_per_rebuild_kernel, dim3((unsigned)groups, M), dim3(per::kRebuildThreads), 0, s, t,
                           groups, (int)run);
    if (groups > 1)  // the top: the subtree over the runs' roots, the tree's nodes [groups, 2 * groups)
        hipLaunchKernelGGL(drl_pop_per_rebuild_kernel, dim3(1, M), dim3(per::kRebuildThreads), 0, s, t, (int64_t)1,
                           (int)groups);
    return (int)hipGetLastError();
}

int launch_sample(const TreeSetArgs& t, hipStream_t s) {
    hipLaunchKernelGGL(drl_pop_per_sample_kernel, dim3((unsigned)t.members), dim3(per::kSampleThreads), 0, s, t);
    return (int)hipGetLastError();
}

// The population's chain (pop::launch_pop_train) on the drawn rows: rebuild and sample in front, this unit's rows
// and TD kernels in place of the uniform ones, the priorities behind the TD; every other launch is the
// population's own kernel with the population's arguments (a.p).
int launch_train(const ChainArgs& a, hipStream_t s) {
    const ll::Plan& P = a.p.P;
    const unsigned M = (unsigned)a.p.members;
    if (const int e = launch_rebuild(a.t, s)) return e;
    if (const int e = launch_sample(a.t, s)) return e;
    const unsigned bt = (unsigned)((P.batch + kThreads - 1) / kThreads);
    const int64_t elems = 2 * (int64_t)P.batch * P.in4;
    hipLaunchKernelGGL(drl_pop_per_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads), M), dim3(kThreads), 0,
                       s, a);
    pop::launch_pop_forward(a.p, s);
    hipLaunchKernelGGL(drl_pop_per_td_kernel, dim3(bt, M), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_pop_per_priority_kernel, dim3(bt, M), dim3(kThreads), 0, s, a);
    pop::launch_pop_backward_update(a.p, s);
    pop::launch_pop_counters(a.p, s);
    return (int)hipGetLastError();
}

}  // namespace perpop
}  // namespace drl
