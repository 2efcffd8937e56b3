// dronerl_convper.hip — prioritized experience replay for the conv Q-network's learner (include/dronerl.h
// drl_convnet_dqn_per_train): drl_convnet_dqn_large_train's chain (convlarge/dronerl_convlarge.hip) on the rows the
// priority tree draws (per/dronerl_per.hip), as a fixed chain of stream-ordered launches:
//   rebuild (one or two launches) and sample: per::launch_rebuild and per::launch_sample, the dense learner's
//                            kernels on the same prioritized block; the sampler reads the step from the conv agent
//                            block's counters;
//   1. drl_convnet_dqn_per_rows_kernel, one workgroup per drawn row, the uniform rows kernel's launch shape: the
//      uniform chain's cg::rows_body (convlarge/dronerl_convlarge_chain.h) with the drawn rows as the rows' policy
//      (dronerl_learn_common.h) -- slots[b] in place of dq_sample, the row's weight on its squared error and on
//      the Q head's delta, |d| kept and the slot's leaf zeroed;
//   2-5. the uniform chain's own dense_grad / conv_grad / update / counters kernels
//      (cg::launch_convlarge_grads_update) with the uniform arguments -- the weights have entered through the
//      deltas and the squared errors;
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
    cg::rows_body(a.P, a, full.d, a.P.batch, (int)blockIdx.x, reinterpret_cast<float*>(cper_lds4));
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
    if (a.c.a.trained) {
        if (const int e = per::launch_rebuild(t, s)) return e;
        if (const int e = per::launch_sample(t, sa, a.c.a.ctr, s)) return e;
        hipLaunchKernelGGL(drl_convnet_dqn_per_rows_kernel, dim3((unsigned)P.batch),
                           dim3((unsigned)a.c.t.rows_threads), (size_t)P.row_words * 4, s, a);
    }
    cg::launch_convlarge_grads_update(a.c, s);
    if (a.c.a.trained)
        hipLaunchKernelGGL(drl_convnet_dqn_per_priority_kernel,
                           dim3((unsigned)((P.batch + per::kThreads - 1) / per::kThreads)), dim3(per::kThreads), 0, s,
                           a);
    return (int)hipGetLastError();
}

}  // namespace cper
}  // namespace drl
