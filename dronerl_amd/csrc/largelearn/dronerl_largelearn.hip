// dronerl_largelearn.hip — the DQN learner for dense Q-networks at replay batches up to 4096
// (include/dronerl.h drl_dqn_large_*): one train_jax.py:68-98 learner block, with drl_dqn_train's semantics and
// its arithmetic bit for bit, as a fixed chain of stream-ordered launches (the host API then re-packs the act's
// image with the pack kernel):
//   1. drl_dqn_large_rows_kernel: the rows' slots (dq_sample at the device step), their obs and next_obs decoded
//      to f32 (dq_input), their action, reward and done;
//   2. drl_dqn_large_forward_kernel, once per layer: the online net on obs and the target net on next_obs;
//   3. drl_dqn_large_td_kernel, a thread per row: max_a Q_target, the TD value, (q - td)^2 and the Q head's deltas
//      2 (q - td) / B;
//   4. drl_dqn_large_backward_kernel, once per layer >= 1: dL/dz of the layer below, masked by relu(z) > 0;
//   5. drl_dqn_large_update_kernel: each parameter's gradient as a sum over the rows in row order (the rows staged
//      through LDS in chunks), Adam, the target blend when due (drl_dqn_large_blend_kernel alone in a step without
//      a sample);
//   6. drl_dqn_large_counters_kernel: the loss (rows in order), Adam's count and powers, the epsilon decay,
//      step + 1 -- the only writer of the counters, behind every reader in stream order; it also clears the act
//      image's status vector for the pack launch behind it.
// No workgroup waits for another and no float atomic is used: the result does not depend on scheduling.
//
// The arithmetic order is oracle/dqn_learner.py's: a dot product keeps four partial sums over k mod 4, each in k
// order, combined (s0 + s1) + (s2 + s3), then + bias; the backward pass the same over the output index; every
// batch sum runs over the rows in order from 0.0; no product is contracted into an FMA.  An MFMA sums its K
// products in an order of its own, so this is VALU work.  The two matrix kernels share one tile loop (ll_tile):
// a workgroup takes 64 rows, one per lane, by 16 outputs, four per wave; the rows' operand goes through LDS in
// 128-column chunks (one 16-B read feeds the four partial sums of four outputs) and the weights are read at
// wave-uniform addresses.  Every loop bound is the validated plan's (dronerl_largelearn_layout.h).  The kernels'
// bodies live in dronerl_largelearn_chain.h, which the population's learner (population/) includes too.  The
// prioritized learner (per/dronerl_per.hip) has rows and TD kernels of its own (the same bodies on the drawn
// rows) and launches this unit's forward, backward, update, blend and counters kernels through launch_large_*.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "dronerl_largelearn_layout.h"
#include "dronerl_largelearn_chain.h"  // the kernels' bodies (shared with population/dronerl_population.hip)

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace ll {

// 1. The rows: grid over 2 nets x batch x in4 elements (rows_body).
__global__ void __launch_bounds__(kThreads) drl_dqn_large_rows_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    rows_body(a.P, a, UniformRows{}, a.P.batch, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// 2. Layer l of both nets (blockIdx.y: 0 the online net on obs, 1 the target net on next_obs; forward_body).
__global__ void __launch_bounds__(kTileThreads) drl_dqn_large_forward_kernel(LearnArgs args, int l) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[kTileRows * kChunkStride];
    forward_body(a.P, a, a.P.batch, l, (int)blockIdx.y, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 3. The TD error, a thread per row (td_body).
__global__ void __launch_bounds__(kThreads) drl_dqn_large_td_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    td_body(a.P, a, UniformRows{}, a.P.batch, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// 4. Layer l - 1's deltas from layer l's (l >= 1; backward_body).
__global__ void __launch_bounds__(kTileThreads) drl_dqn_large_backward_kernel(LearnArgs args, int l) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[kTileRows * kChunkStride];
    backward_body(a.P, a, a.P.batch, l, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 5. The parameters: workgroup (blockIdx.x, blockIdx.y) of layer blockIdx.z (update_body): the gradient, Adam,
// the target blend when due.
__global__ void __launch_bounds__(kUpdateThreads) drl_dqn_large_update_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[kUpdateChunk * kUpdateCols];
    __shared__ __attribute__((aligned(16))) float Ds[kUpdateChunk * kUpdateUnits];
    update_body(a.P, a, a.P.batch, (int)blockIdx.z, (int)blockIdx.x, (int)blockIdx.y, Xs, Ds);
}

// A step without a sample (buffer.can_sample is false): no train_step; the target blend when due, over the
// whole set as drl_dqn_train does it.
__global__ void __launch_bounds__(kThreads) drl_dqn_large_blend_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.P.n_params) return;
    blend_body(a, i);
}

// 6. The counters (one workgroup; counters_body).
__global__ void __launch_bounds__(kThreads) drl_dqn_large_counters_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& a = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float sq[kMaxBatch];
    // the act image's status vector, cleared for the pack launch that follows (a store, not a memset: a
    // captured call then holds kernel nodes only, as the conv learner's)
    if (threadIdx.x < 4) a.pack_status[threadIdx.x] = 0u;
    counters_body(a.P, a, a.P.batch, a.trained, sq);
}

// The replay slots the next drl_dqn_large_train launch samples (its step counter as it stands on the stream)
__global__ void __launch_bounds__(kThreads) drl_dqn_large_sample_kernel(const DqnCounters* c, uint64_t seed,
                                                                        int batch, int64_t size, int64_t* out) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b < batch) out[b] = dq_sample(seed, c->step, b, size);
}

// ---- the chain's segments: the launches a prioritized chain (per/dronerl_per.hip) takes over as they are.  The
// grid arithmetic lives here alone; the caller reads hipGetLastError behind its last launch.
// 1. the rows (uniform draws), and the grid every chain's TD kernel takes: a thread per row
void launch_large_rows(const LearnArgs& a, hipStream_t s) {
    const int64_t elems = 2 * (int64_t)a.P.batch * a.P.in4;
    hipLaunchKernelGGL(drl_dqn_large_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       s, a);
}

// 2. every layer's forward
void launch_large_forward(const LearnArgs& a, hipStream_t s) {
    const Plan& P = a.P;
    for (int l = 0; l < P.n_layers; ++l)
        hipLaunchKernelGGL(drl_dqn_large_forward_kernel, dim3((unsigned)row_tiles(P), 2, (unsigned)unit_tiles(P.out[l])),
                           dim3(kTileThreads), 0, s, a, l);
}

// 4.-5. the backward pass of every layer >= 1, then the update
void launch_large_backward_update(const LearnArgs& a, hipStream_t s) {
    const Plan& P = a.P;
    const int L = P.n_layers;
    for (int l = L - 1; l >= 1; --l)
        hipLaunchKernelGGL(drl_dqn_large_backward_kernel, dim3((unsigned)row_tiles(P), 1, (unsigned)unit_tiles(P.in[l])),
                           dim3(kTileThreads), 0, s, a, l);
    int kt = 0, jt = 0;  // (the widest layer's tiles; a workgroup outside its layer's returns at once)
    for (int l = 0; l < L; ++l) {
        kt = update_col_tiles(P, l) > kt ? update_col_tiles(P, l) : kt;
        jt = update_unit_tiles(P, l) > jt ? update_unit_tiles(P, l) : jt;
    }
    hipLaunchKernelGGL(drl_dqn_large_update_kernel, dim3((unsigned)kt, (unsigned)jt, (unsigned)L),
                       dim3(kUpdateThreads), 0, s, a);
}

// a step without a sample: the blend
void launch_large_blend(const LearnArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_dqn_large_blend_kernel, dim3((unsigned)((a.P.n_params + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, a);
}

// 6. the counters
void launch_large_counters(const LearnArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_dqn_large_counters_kernel, dim3(1), dim3(kThreads), 0, s, a);
}

int launch_large_train(const LearnArgs& a, hipStream_t s) {
    const Plan& P = a.P;
    const dim3 eb(kThreads);
    if (a.trained) {
        launch_large_rows(a, s);
        launch_large_forward(a, s);
        hipLaunchKernelGGL(drl_dqn_large_td_kernel, dim3((unsigned)((P.batch + kThreads - 1) / kThreads)), eb, 0, s, a);
        launch_large_backward_update(a, s);
    } else {
        launch_large_blend(a, s);
    }
    launch_large_counters(a, s);
    return (int)hipGetLastError();
}

int launch_large_sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(drl_dqn_large_sample_kernel, dim3((unsigned)((batch + kThreads - 1) / kThreads)), dim3(kThreads),
                       0, s, static_cast<const DqnCounters*>(counters), seed, batch, size, out);
    return (int)hipGetLastError();
}

}  // namespace ll
}  // namespace drl
