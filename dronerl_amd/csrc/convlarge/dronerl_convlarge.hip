// dronerl_convlarge.hip — the DQN learner for conv Q-networks at replay batches up to 4096 (include/dronerl.h
// drl_convnet_dqn_large_*): one train_jax.py:68-98 learner block with network_type == 'conv', with
// drl_convnet_dqn_train's semantics, as a fixed chain of stream-ordered launches (the host API then re-packs the
// act's image with the pack kernel):
//   1. drl_convnet_dqn_large_rows_kernel, one workgroup per sampled row (256 threads; up to 1024, by the widest
//      layer, at batches up to 512: a row's arithmetic does not depend on the count): drl_convnet_dqn_rows_kernel's row (the target net
//      on next_obs, the online net on obs, the TD error, the head's deltas 2 (q - td) / B with the full batch B,
//      the backward pass to every layer's dL/dz; convlearn/dronerl_convlearn_rows.h), to the scratch;
//   2. drl_convnet_dqn_large_dense_grad_kernel: the rows are cut into chunks of 64 (chunk c: rows 64 c ..), and a
//      workgroup takes (chunk, 32 units, 64 columns of [W_l | b_l]) of a dense layer: the chunk's deltas and
//      inputs staged once in LDS, a thread keeps 8 units of one column in registers and adds the chunk's rows in
//      row order from 0.0 -- the chunk's partial gradient, to the scratch;
//   3. drl_convnet_dqn_large_conv_grad_kernel, one wave per (chunk, conv parameter group: the k x k weights of
//      one (co, ci), or one bias): each parameter's chunk terms (row, position) dealt to the lanes by
//      (b hw + pos) mod 64, each lane's in t order, then the fixed xor tree -- what
//      drl_convnet_dqn_update_kernel does for its whole batch;
//   4. drl_convnet_dqn_large_update_kernel, one thread per parameter: g = p[0] + p[1] + ... in chunk order, Adam,
//      the target blend when due (in a step without a sample: the blend alone);
//   5. drl_convnet_dqn_large_counters_kernel: the loss (each chunk's squared errors in row order, the chunk sums
//      in chunk order, / B), Adam's count and powers, the epsilon decay, step + 1 -- the only writer of the
//      counters, behind every reader in stream order; it also clears the act image's status vector for the pack
//      launch behind it.
// No workgroup waits for another and no float atomic is used: the result does not depend on scheduling.  With
// one chunk (B <= 64) every sum is drl_convnet_dqn_train's own, so the two learners agree bit for bit.  An MFMA
// sums its K products in an order of its own, so the partials are VALU work.  Every loop bound is the validated
// plan's (dronerl_convlarge_layout.h).  The kernels' bodies live in dronerl_convlarge_chain.h, which the
// population's kernels (convpop/dronerl_convpop.hip) run too.  The prioritized learner (convper/) has a rows kernel
// of its own (the same body on the drawn rows) and launches this unit's kernels 2.-5. behind it
// (launch_convlarge_grads_update).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "../convlearn/dronerl_convlearn_rows.h"
#include "dronerl_convlarge_chain.h"
#include "dronerl_convlarge_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace cg {

// The bodies are dronerl_convlarge_chain.h's (shared with the population's kernels, convpop/): each kernel here
// passes its LearnArgs, the plan's batch and its workgroup coordinates.

// 1. The rows: one workgroup per sampled row.
__global__ void __launch_bounds__(kRowsThreadsMax) drl_convnet_dqn_large_rows_kernel(LearnArgs args) {
    // (the arguments read in place from the kernarg segment: indexing a by-value copy's layers at run time
    // would move it to private memory)
    (void)args;
    const cl::LearnArgs& a = ((const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr())->a;
    extern __shared__ float4 cg_lds4[];
    rows_body(a.P, a, UniformRows{}, a.P.batch, (int)blockIdx.x, reinterpret_cast<float*>(cg_lds4));
}

// 2. A dense layer's chunk partials: workgroup (tile blockIdx.x, chunk blockIdx.y).
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_dense_grad_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[kChunkRows * kTileCols];
    __shared__ __attribute__((aligned(16))) float Ds[kChunkRows * kTileUnits];
    const int c = blockIdx.y;
    if (c >= full.t.chunks || (int)blockIdx.x >= full.t.dense_tiles) return;
    dense_grad_body(full.a.P, full.t, full.a, full.a.P.batch, (int)blockIdx.x, c, Xs, Ds);
}

// 3. The conv layers' chunk partials: wave (parameter group, chunk blockIdx.y), kConvWaves groups per workgroup.
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_conv_grad_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int c = blockIdx.y;
    const int gi = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kConvWaves + (int)(threadIdx.x >> 6));
    if (gi >= full.t.conv_groups || c >= full.t.chunks) return;  // (the whole wave)
    conv_grad_body(full.a.P, full.t, full.a, full.a.P.batch, gi, c);
}

// 4. The parameters, a thread each: the chunk partials in chunk order, Adam, the target blend when due.
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_update_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    update_body(full.a.P, full.t, full.a, full.a.trained, full.t.chunks, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// 5. The counters (one wave); it also clears the act image's status vector for the pack launch behind it.
__global__ void __launch_bounds__(64) drl_convnet_dqn_large_counters_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float cs[kMaxChunks];
    counters_body(full.a.P, full.a, full.a.P.batch, full.a.trained, full.t.chunks, full.a.pack_status, cs);
}

// The replay slots the next drl_convnet_dqn_large_train launch samples (its step counter as it stands on the
// stream)
__global__ void __launch_bounds__(kThreads) drl_convnet_dqn_large_sample_kernel(const DqnCounters* c, uint64_t seed,
                                                                                int batch, int64_t size,
                                                                                int64_t* out) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b < batch) out[b] = dq_sample(seed, c->step, b, size);
}

// 2.-5. Everything behind the rows: the chunk partials (with a sample), the update, the counters.  The prioritized
// chain (convper/dronerl_convper.hip) launches these as they are behind its own rows kernel; the caller reads
// hipGetLastError behind its last launch.
void launch_convlarge_grads_update(const LearnArgs& a, hipStream_t s) {
    const cl::Plan& P = a.a.P;
    const unsigned chunks = (unsigned)a.t.chunks;
    if (a.a.trained) {
        hipLaunchKernelGGL(drl_convnet_dqn_large_dense_grad_kernel, dim3((unsigned)a.t.dense_tiles, chunks),
                           dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(drl_convnet_dqn_large_conv_grad_kernel,
                           dim3((unsigned)((a.t.conv_groups + kConvWaves - 1) / kConvWaves), chunks), dim3(kThreads),
                           0, s, a);
    }
    hipLaunchKernelGGL(drl_convnet_dqn_large_update_kernel, dim3((unsigned)((P.n_params + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_convnet_dqn_large_counters_kernel, dim3(1), dim3(64), 0, s, a);
}

int launch_convlarge_train(const LearnArgs& a, hipStream_t s) {
    const cl::Plan& P = a.a.P;
    if (a.a.trained)
        hipLaunchKernelGGL(drl_convnet_dqn_large_rows_kernel, dim3((unsigned)P.batch),
                           dim3((unsigned)a.t.rows_threads), (size_t)P.row_words * 4, s, a);
    launch_convlarge_grads_update(a, s);
    return (int)hipGetLastError();
}

int launch_convlarge_sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(drl_convnet_dqn_large_sample_kernel, dim3((unsigned)((batch + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, static_cast<const DqnCounters*>(counters), seed, batch, size, out);
    return (int)hipGetLastError();
}

}  // namespace cg
}  // namespace drl
