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
//   drl_pop_per_rows / forward / td / priority / backward / update / counters _kernel
//                                the large-batch learner's chain (largelearn/dronerl_largelearn_chain.h) with the
//                                prioritized rows, TD and priority bodies of per/dronerl_per_chain.h -- the
//                                bodies drl_dqn_per_train's kernels run -- a member per grid slice.
// A member trains iff size >= its batch, decided here on the device from its hyperparameter record, as in
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
#include "dronerl_perpop_layout.h"

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {
namespace perpop {

namespace {

// A member's view: the fields the chain's bodies and dronerl_learn_common.h read (ll::LearnArgs' names) and the
// prioritized bodies' (per::LearnArgs' names).
struct Member {
    int32_t batch, code_w;
    float* online;
    float* target;
    float* adam_m;
    float* adam_v;
    DqnCounters* ctr;
    float* scratch;
    const uint32_t* r_obs;
    const uint32_t* r_next;
    int64_t row_words;
    const int32_t* r_act;
    const float* r_rew;
    const uint8_t* r_done;
    int64_t size;
    uint64_t seed;
    float gamma, b1, b2, c1, c2, adam_eps, neg_lr, tau, one_minus_tau, eps_decay, eps_end;
    double b1d, b2d;
    int32_t target_every, eps_every;
    const int64_t* slots;
    const float* weights;
    float* absd;
    float* leaves;
    float* pmax;
    double alpha, per_eps;
};

__device__ __forceinline__ const pop::HRec& hrec(const uint8_t* pop_base, int64_t hp_off, int m) {
    return *reinterpret_cast<const pop::HRec*>(pop_base + hp_off + pop::kHRecStride * m);
}

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

__device__ __forceinline__ Member member_of(const ChainArgs& c, int m) {
    const pop::PopArgs& a = c.p;
    const ll::Plan& P = a.P;
    uint8_t* blk = a.base + a.stride * m;
    const pop::HRec& h = hrec(a.base, a.hp_off, m);
    Member v;
    v.batch = h.batch;
    v.code_w = P.code_w;
    v.online = reinterpret_cast<float*>(blk + P.pub.online_off);
    v.target = reinterpret_cast<float*>(blk + P.pub.target_off);
    v.adam_m = reinterpret_cast<float*>(blk + P.pub.m_off);
    v.adam_v = reinterpret_cast<float*>(blk + P.pub.v_off);
    v.ctr = reinterpret_cast<DqnCounters*>(blk + P.pub.counters_off);
    v.scratch = reinterpret_cast<float*>(blk + P.pub.scratch_off);
    const int64_t r0 = a.capacity * m;
    v.r_obs = a.r_obs + r0 * a.row_words;
    v.r_next = a.r_next + r0 * a.row_words;
    v.row_words = a.row_words;
    v.r_act = a.r_act + r0;
    v.r_rew = a.r_rew + r0;
    v.r_done = a.r_done + r0;
    v.size = a.size;
    v.seed = h.seed;
    v.gamma = h.gamma;
    v.b1 = h.b1;
    v.b2 = h.b2;
    v.c1 = h.c1;
    v.c2 = h.c2;
    v.adam_eps = h.adam_eps;
    v.neg_lr = h.neg_lr;
    v.tau = h.tau;
    v.one_minus_tau = h.one_minus_tau;
    v.eps_decay = h.eps_decay;
    v.eps_end = h.eps_end;
    v.b1d = h.b1d;
    v.b2d = h.b2d;
    v.target_every = h.target_every;
    v.eps_every = h.eps_every;
    const per::TreeArgs t = tree_of(c.t, m, h.batch);
    const PRec& pr = prec(c.t, m);
    v.slots = t.slots;
    v.weights = t.weights;
    v.absd = t.absd;
    v.leaves = t.tree + t.P;
    v.pmax = t.pmax;
    v.alpha = pr.alpha;
    v.per_eps = pr.eps;
    return v;
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

// ---- the learner: the prioritized chain with the member in the grid --------------------------------------------
// 1. rows: grid (elements of 2 x max_batch x in4, members)
__global__ void __launch_bounds__(kThreads) drl_pop_per_rows_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Member v = member_of(a, blockIdx.y);
    if (a.p.size < v.batch) return;
    per::per_rows_body(a.p.P, v, v.batch, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// 2. layer l's forward: grid (row tiles, 2 nets x members, unit tiles)
__global__ void __launch_bounds__(ll::kTileThreads) drl_pop_per_forward_kernel(ChainArgs args, int l) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    const Member v = member_of(a, blockIdx.y >> 1);
    if (a.p.size < v.batch || (int)blockIdx.x * ll::kTileRows >= v.batch) return;  // (uniform over the workgroup)
    ll::forward_body(a.p.P, v, v.batch, l, (int)(blockIdx.y & 1), (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 3. TD: grid (max_batch rows, members); the head's deltas divide by the member's batch
__global__ void __launch_bounds__(kThreads) drl_pop_per_td_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Member v = member_of(a, blockIdx.y);
    if (a.p.size < v.batch) return;
    per::per_td_body(a.p.P, v, v.batch, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// 4. the priorities: grid (max_batch rows, members), into the member's leaves and its pmax
__global__ void __launch_bounds__(kThreads) drl_pop_per_priority_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ uint32_t wg_max;
    const Member v = member_of(a, blockIdx.y);
    if (a.p.size < v.batch || (int)(blockIdx.x * kThreads) >= v.batch) return;  // (uniform over the workgroup)
    per::priority_body(v, v.batch, (int)(blockIdx.x * kThreads + threadIdx.x), &wg_max);
}

// 5. layer l's backward (l >= 1): grid (row tiles, members, unit tiles)
__global__ void __launch_bounds__(ll::kTileThreads) drl_pop_per_backward_kernel(ChainArgs args, int l) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    const Member v = member_of(a, blockIdx.y);
    if (a.p.size < v.batch || (int)blockIdx.x * ll::kTileRows >= v.batch) return;
    ll::backward_body(a.p.P, v, v.batch, l, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 6. update: grid (column tiles, unit tiles, layers x members).  A member that does not train blends its target
// when due: each thread the two parameters it would have updated (drl_pop_update_kernel's rule).
__global__ void __launch_bounds__(ll::kUpdateThreads) drl_pop_per_update_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const ll::Plan& P = a.p.P;
    __shared__ __attribute__((aligned(16))) float Xs[ll::kUpdateChunk * ll::kUpdateCols];
    __shared__ __attribute__((aligned(16))) float Ds[ll::kUpdateChunk * ll::kUpdateUnits];
    const int L = P.n_layers;
    const int m = blockIdx.z / L, l = blockIdx.z - m * L;
    const Member v = member_of(a, m);
    if (a.p.size >= v.batch) {
        ll::update_body(P, v, v.batch, l, (int)blockIdx.x, (int)blockIdx.y, Xs, Ds);
        return;
    }
    const int k = blockIdx.x * ll::kUpdateCols + (threadIdx.x & (ll::kUpdateCols - 1));
    const int j = blockIdx.y * ll::kUpdateUnits + 2 * (threadIdx.x / ll::kUpdateCols);
    for (int u = 0; u < 2; ++u) {
        const int64_t i = ll::update_param(P, l, j + u, k);
        if (i >= 0) ll::blend_body(v, i);
    }
}

// 7. counters: a workgroup per member
__global__ void __launch_bounds__(kThreads) drl_pop_per_counters_kernel(ChainArgs args) {
    (void)args;
    const ChainArgs& a = *(const ChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float sq[ll::kMaxBatch];
    const Member v = member_of(a, blockIdx.x);
    ll::counters_body(a.p.P, v, v.batch, a.p.size >= v.batch ? 1 : 0, sq);
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

int launch_train(const ChainArgs& a, hipStream_t s) {
    const ll::Plan& P = a.p.P;
    const unsigned M = (unsigned)a.p.members;
    const int L = P.n_layers;
    if (const int e = launch_rebuild(a.t, s)) return e;
    if (const int e = launch_sample(a.t, s)) return e;
    const unsigned rt = (unsigned)ll::row_tiles(P), bt = (unsigned)((P.batch + kThreads - 1) / kThreads);
    const int64_t elems = 2 * (int64_t)P.batch * P.in4;
    hipLaunchKernelGGL(drl_pop_per_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads), M), dim3(kThreads), 0,
                       s, a);
    for (int l = 0; l < L; ++l)
        hipLaunchKernelGGL(drl_pop_per_forward_kernel, dim3(rt, 2 * M, (unsigned)ll::unit_tiles(P.out[l])),
                           dim3(ll::kTileThreads), 0, s, a, l);
    hipLaunchKernelGGL(drl_pop_per_td_kernel, dim3(bt, M), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_pop_per_priority_kernel, dim3(bt, M), dim3(kThreads), 0, s, a);
    for (int l = L - 1; l >= 1; --l)
        hipLaunchKernelGGL(drl_pop_per_backward_kernel, dim3(rt, M, (unsigned)ll::unit_tiles(P.in[l])),
                           dim3(ll::kTileThreads), 0, s, a, l);
    int kt = 0, jt = 0;  // (the widest layer's tiles; a workgroup outside its layer's returns at once)
    for (int l = 0; l < L; ++l) {
        kt = ll::update_col_tiles(P, l) > kt ? ll::update_col_tiles(P, l) : kt;
        jt = ll::update_unit_tiles(P, l) > jt ? ll::update_unit_tiles(P, l) : jt;
    }
    hipLaunchKernelGGL(drl_pop_per_update_kernel, dim3((unsigned)kt, (unsigned)jt, (unsigned)L * M),
                       dim3(ll::kUpdateThreads), 0, s, a);
    hipLaunchKernelGGL(drl_pop_per_counters_kernel, dim3(M), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace perpop
}  // namespace drl
