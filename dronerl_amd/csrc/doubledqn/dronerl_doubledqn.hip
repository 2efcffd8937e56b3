// dronerl_doubledqn.hip — Double DQN targets (van Hasselt et al. 2016) for the dense learners' launch chains
// (include/dronerl.h drl_dqn_double_train, drl_widenet_dqn_double_train, their prioritized variants and
// drl_pop_double_train).  A step is the max-rule chain's (largelearn/, per/, population/) with one change in the
// TD rule: the next state's value is the target net's at the ONLINE net's first maximum on next_obs,
//   qs = Q_online(next_obs_b);  a* = argmax qs (the first maximum; a NaN never wins);  td = r + gamma qt[a*] (1 - done)
// which takes a third forward pass per row, the selector.  It needs no scratch of its own: layer l's selector
// activations live in the delta words d_off[l], which nothing reads between the rows launch and the TD launch
// (DESIGN.md §4 has the table of who writes and who reads them).  It needs no launch of its own either:
//   drl_dqn_double_forward_kernel   the chain's forward with a third blockIdx.y slice (ll::selector_body: the
//                                   same tile loop, LDS and launch bounds on other pointers);
//   drl_dqn_double_td_kernel        ll::td_body under DoubleTarget on uniform rows: the selector's Q values read
//   drl_dqn_double_per_td_kernel    into registers, then the deltas stored over them; the same on drawn rows;
//   drl_pop_double_forward_kernel   the population's: grid (row tiles, 3 x members, unit tiles), and a device byte
//   drl_pop_double_td_kernel        per member: 0 = the member's selector slice returns at once and its TD runs
//                                   MaxTarget (uniform over the workgroup).
// Every other launch of a step is the max-rule chain's own kernel through its launch_* segments, so a Double
// step has exactly the launches of the max-rule step.  Kernel nodes only, no workgroup waits for another, no
// float atomic: nothing depends on scheduling, and a step is graph-capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "../largelearn/dronerl_largelearn_chain.h"
#include "../per/dronerl_per_layout.h"
#include "../population/dronerl_population_layout.h"
#include "../population/dronerl_population_member.h"
#include "dronerl_doubledqn.h"

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {
namespace dd {

// ---- one agent ---------------------------------------------------------------------------------------------------
// 2. Layer l: blockIdx.y 0 the online net on obs, 1 the target net on next_obs (ll::forward_body), 2 the selector,
// the online net on next_obs (ll::selector_body).
__global__ void __launch_bounds__(ll::kTileThreads) drl_dqn_double_forward_kernel(ll::LearnArgs args, int l) {
    (void)args;
    const ll::LearnArgs& a = *(const ll::LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    if (blockIdx.y < 2)
        ll::forward_body(a.P, a, a.P.batch, l, (int)blockIdx.y, (int)blockIdx.x, (int)blockIdx.z, Xs);
    else
        ll::selector_body(a.P, a, a.P.batch, l, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 3. The TD error under DoubleTarget, a thread per row: uniform rows ...
__global__ void __launch_bounds__(kThreads) drl_dqn_double_td_kernel(ll::LearnArgs args) {
    (void)args;
    const ll::LearnArgs& a = *(const ll::LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    ll::td_body(a.P, a, UniformRows{}, a.P.batch, (int)(blockIdx.x * kThreads + threadIdx.x), DoubleTarget{});
}

// ... and the prioritized replay's drawn rows (the row's weight, |d| kept, the slot's leaf zeroed)
__global__ void __launch_bounds__(kThreads) drl_dqn_double_per_td_kernel(per::LearnArgs args) {
    (void)args;
    const per::LearnArgs& a = *(const per::LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    ll::td_body(a.P, a, a.d, a.P.batch, (int)(blockIdx.x * kThreads + threadIdx.x), DoubleTarget{});
}

// ---- the population: the rule per member -------------------------------------------------------------------------
// 2. layer l's forward: grid (row tiles, 3 passes x members, unit tiles)
__global__ void __launch_bounds__(ll::kTileThreads) drl_pop_double_forward_kernel(PopArgs args, int l) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    const int m = blockIdx.y / 3, n = blockIdx.y - 3 * m;
    if (n == 2 && !a.dbl[m]) return;  // a max-rule member has no selector (uniform over the workgroup)
    const pop::Member v = pop::member_of(a, m);
    if (a.size < v.batch || (int)blockIdx.x * ll::kTileRows >= v.batch) return;  // (uniform over the workgroup)
    if (n < 2)
        ll::forward_body(a.P, v, v.batch, l, n, (int)blockIdx.x, (int)blockIdx.z, Xs);
    else
        ll::selector_body(a.P, v, v.batch, l, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 3. TD: grid (max_batch rows, members); the member's rule
__global__ void __launch_bounds__(kThreads) drl_pop_double_td_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const pop::Member v = pop::member_of(a, blockIdx.y);
    if (a.size < v.batch) return;
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (a.dbl[blockIdx.y])
        ll::td_body(a.P, v, UniformRows{}, v.batch, b, DoubleTarget{});
    else
        ll::td_body(a.P, v, UniformRows{}, v.batch, b, MaxTarget{});
}

// ---- launches ----------------------------------------------------------------------------------------------------
namespace {

// 2. every layer's forward, three passes
void launch_double_forward(const ll::LearnArgs& a, hipStream_t s) {
    const ll::Plan& P = a.P;
    for (int l = 0; l < P.n_layers; ++l)
        hipLaunchKernelGGL(drl_dqn_double_forward_kernel,
                           dim3((unsigned)ll::row_tiles(P), 3, (unsigned)ll::unit_tiles(P.out[l])),
                           dim3(ll::kTileThreads), 0, s, a, l);
}

}  // namespace

// ll::launch_large_train with this unit's forward and TD kernels
int launch_double_train(const ll::LearnArgs& a, hipStream_t s) {
    if (a.trained) {
        ll::launch_large_rows(a, s);
        launch_double_forward(a, s);
        hipLaunchKernelGGL(drl_dqn_double_td_kernel, dim3((unsigned)((a.P.batch + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, s, a);
        ll::launch_large_backward_update(a, s);
    } else {
        ll::launch_large_blend(a, s);
    }
    ll::launch_large_counters(a, s);
    return (int)hipGetLastError();
}

// per::launch_per_train with this unit's forward and TD kernels
int launch_double_per_train(const per::LearnArgs& a, const per::TreeArgs& t, const per::SampleArgs& sa,
                            hipStream_t s) {
    if (a.trained) {
        if (const int e = per::launch_rebuild(t, s)) return e;
        if (const int e = per::launch_sample(t, sa, a.ctr, s)) return e;
        per::launch_per_rows(a, s);
        launch_double_forward(a, s);
        hipLaunchKernelGGL(drl_dqn_double_per_td_kernel, dim3((unsigned)((a.P.batch + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, s, a);
        per::launch_per_priority(a, s);
        ll::launch_large_backward_update(a, s);
    } else {
        ll::launch_large_blend(a, s);
    }
    ll::launch_large_counters(a, s);
    return (int)hipGetLastError();
}

// pop::launch_pop_train with this unit's forward and TD kernels
int launch_pop_double_train(const PopArgs& a, hipStream_t s) {
    const ll::Plan& P = a.P;
    const unsigned M = (unsigned)a.members;
    pop::launch_pop_rows(a, s);
    for (int l = 0; l < P.n_layers; ++l)
        hipLaunchKernelGGL(drl_pop_double_forward_kernel,
                           dim3((unsigned)ll::row_tiles(P), 3 * M, (unsigned)ll::unit_tiles(P.out[l])),
                           dim3(ll::kTileThreads), 0, s, a, l);
    hipLaunchKernelGGL(drl_pop_double_td_kernel, dim3((unsigned)((P.batch + kThreads - 1) / kThreads), M), dim3(kThreads),
                       0, s, a);
    pop::launch_pop_backward_update(a, s);
    pop::launch_pop_counters(a, s);
    return (int)hipGetLastError();
}

}  // namespace dd
}  // namespace drl
