// dronerl_convper.hip — prioritized experience replay for the conv Q-network's learner (include/dronerl.h
// drl_convnet_dqn_per_train): drl_convnet_dqn_large_train's chain (convlarge/dronerl_convlarge.hip) on the rows the
// priority tree draws (per/dronerl_per.hip), as a fixed chain of stream-ordered launches:
//   rebuild (one or two launches) and sample: per::launch_rebuild and per::launch_sample, the dense learner's
//                            kernels on the same prioritized block; the sampler reads the step from the conv agent
//                            block's counters;
//   1. drl_convnet_dqn_per_rows_kernel, one workgroup per drawn row, the uniform rows kernel's launch shape:
//      per_rows_body (dronerl_convper_chain.h) -- cg::rows_body with slots[b] in place of dq_sample, the row's
//      weight on its squared error and on the Q head's delta, |d| kept and the slot's leaf zeroed;
//   2-5. drl_convnet_dqn_per_dense_grad / conv_grad / update / counters _kernel: the uniform chain's bodies
//      (convlarge/dronerl_convlarge_chain.h) as they are -- the weights have entered through the deltas and the
//      squared errors;
//   6. drl_convnet_dqn_per_priority_kernel: per::priority_body -- each drawn leaf raised to its rows' largest new
//      priority with an integer max on the float's bits, and pmax the same way.  It runs behind the rows kernel,
//      which zeroed the leaves, and before the next step's rebuild.
// With size < batch: the update's blend-only path and the counters; the tree is not touched and nothing is drawn.
// No workgroup waits for another and no float atomic is used: nothing depends on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "../convlearn/dronerl_convlearn_rows.h"
#include "../convlarge/dronerl_convlarge_chain.h"
#include "../per/dronerl_per_chain.h"
#include "dronerl_convper_chain.h"
#include "dronerl_convper_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace cper {

// 1. The rows: one workgroup per drawn row.
__global__ void __launch_bounds__(cg::kRowsThreadsMax) drl_convnet_dqn_per_rows_kernel(LearnArgs args) {
    // (the arguments read in place from the kernarg segment, as drl_convnet_dqn_large_rows_kernel reads them)
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::LearnArgs& a = full.c.a;
    extern __shared__ float4 cper_lds4[];
    per_rows_body(a.P, a, full.d, a.P.batch, (int)blockIdx.x, reinterpret_cast<float*>(cper_lds4));
}

// 2. A dense layer's chunk partials: workgroup (tile blockIdx.x, chunk blockIdx.y).
__global__ void __launch_bounds__(cg::kThreads) drl_convnet_dqn_per_dense_grad_kernel(LearnArgs args) {
    (void)args;
    const cg::LearnArgs& full = ((const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr())->c;
    __shared__ __attribute__((aligned(16))) float Xs[cg::kChunkRows * cg::kTileCols];
    __shared__ __attribute__((aligned(16))) float Ds[cg::kChunkRows * cg::kTileUnits];
    const int c = blockIdx.y;
    if (c >= full.t.chunks || (int)blockIdx.x >= full.t.dense_tiles) return;
    cg::dense_grad_body(full.a.P, full.t, full.a, full.a.P.batch, (int)blockIdx.x, c, Xs, Ds);
}

// 3. The conv layers' chunk partials: wave (parameter group, chunk blockIdx.y), kConvWaves groups per workgroup.
__global__ void __launch_bounds__(cg::kThreads) drl_convnet_dqn_per_conv_grad_kernel(LearnArgs args) {
    (void)args;
    const cg::LearnArgs& full = ((const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr())->c;
    const int c = blockIdx.y;
    const int gi = __builtin_amdgcn_readfirstlane((int)blockIdx.x * cg::kConvWaves + (int)(threadIdx.x >> 6));
    if (gi >= full.t.conv_groups || c >= full.t.chunks) return;  // (the whole wave)
    cg::conv_grad_body(full.a.P, full.t, full.a, full.a.P.batch, gi, c);
}

// 4. The parameters, a thread each: the chunk partials in chunk order, Adam, the target blend when due.
__global__ void __launch_bounds__(cg::kThreads) drl_convnet_dqn_per_update_kernel(LearnArgs args) {
    (void)args;
    const cg::LearnArgs& full = ((const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr())->c;
    cg::update_body(full.a.P, full.t, full.a, full.a.trained, full.t.chunks,
                    (int64_t)blockIdx.x * cg::kThreads + threadIdx.x);
}

// 5. The counters (one wave); it also clears the act image's status vector for the pack launch behind it.
__global__ void __launch_bounds__(64) drl_convnet_dqn_per_counters_kernel(LearnArgs args) {
    (void)args;
    const cg::LearnArgs& full = ((const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr())->c;
    __shared__ float cs[cg::kMaxChunks];
    cg::counters_body(full.a.P, full.a, full.a.P.batch, full.a.trained, full.t.chunks, full.a.pack_status, cs);
}

// 6. The priorities (per::priority_body): each drawn leaf raised to its rows' largest new priority, and pmax.
__global__ void __launch_bounds__(per::kThreads) drl_convnet_dqn_per_priority_kernel(LearnArgs args) {
    (void)args;
    const LearnArgs& full = *(const LearnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ uint32_t wg_max;
    per::priority_body(full.d, full.c.a.P.batch, (int)(blockIdx.x * per::kThreads + threadIdx.x), &wg_max);
}

int launch_convper_train(const LearnArgs& a, const per::TreeArgs& t, const per::SampleArgs& sa, hipStream_t s) {
    const cl::Plan& P = a.c.a.P;
    const cg::Tiles& T = a.c.t;
    const unsigned chunks = (unsigned)T.chunks;
    if (a.c.a.trained) {
        if (const int e = per::launch_rebuild(t, s)) return e;
        if (const int e = per::launch_sample(t, sa, a.c.a.ctr, s)) return e;
        hipLaunchKernelGGL(drl_convnet_dqn_per_rows_kernel, dim3((unsigned)P.batch), dim3((unsigned)T.rows_threads),
                           (size_t)P.row_words * 4, s, a);
        hipLaunchKernelGGL(drl_convnet_dqn_per_dense_grad_kernel, dim3((unsigned)T.dense_tiles, chunks),
                           dim3(cg::kThreads), 0, s, a);
        hipLaunchKernelGGL(drl_convnet_dqn_per_conv_grad_kernel,
                           dim3((unsigned)((T.conv_groups + cg::kConvWaves - 1) / cg::kConvWaves), chunks),
                           dim3(cg::kThreads), 0, s, a);
    }
    hipLaunchKernelGGL(drl_convnet_dqn_per_update_kernel,
                       dim3((unsigned)((P.n_params + cg::kThreads - 1) / cg::kThreads)), dim3(cg::kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_convnet_dqn_per_counters_kernel, dim3(1), dim3(64), 0, s, a);
    if (a.c.a.trained)
        hipLaunchKernelGGL(drl_convnet_dqn_per_priority_kernel,
                           dim3((unsigned)((P.batch + per::kThreads - 1) / per::kThreads)), dim3(per::kThreads), 0, s,
                           a);
    return (int)hipGetLastError();
}

}  // namespace cper
}  // namespace drl
