// dronerl_convper_chain.h — the one body the prioritized conv learner adds to the conv large-batch chain (device
// only): a drawn row.  It is cg::rows_body (convlarge/dronerl_convlarge_chain.h) with the slot the sampler drew
// in place of dq_sample and per::per_td_body's TD stores (per/dronerl_per_chain.h): the row's importance weight on
// its squared error and on the Q head's delta, |d| kept for the priority kernel and the slot's leaf zeroed.  It
// takes the agent view `a` (cl::LearnArgs' field names) and the drawn rows' view `p` (cper::Drawn's field names),
// so a prioritized conv population can pass a member's views.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_learn_common.h"
#include "../convlearn/dronerl_convlearn_rows.h"
#include "../convlarge/dronerl_convlarge_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace cper {

namespace {

// Row b of the batch (one workgroup, the row's words in LDS).  With a weight of 1.0 every store is
// cg::rows_body's bit for bit (1.0f * x == x).
template <class V, class D>
__device__ __forceinline__ void per_rows_body(const cl::Plan& P, const V& a, const D& p, int batch, int b,
                                              float* row) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (b >= batch) return;
    const int L = P.n_layers, A = P.n_actions;
    const int64_t s = p.slots[b];
    for (int i = tid; i < P.row_words; i += nt) row[i] = 0.0f;
    __syncthreads();
    // the target net on next_obs: max_a Q_target
    for (int i = tid; i < P.in; i += nt) row[i] = dq_input(a, a.r_next, s, i);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        cl::cl_forward(P, l, a.target, row);
        __syncthreads();
    }
    const float* qv = row + P.l[L - 1].delta;
    float mx = 0.0f;  // (thread 0 alone forms the TD error: it keeps the maximum in a register)
    if (tid == 0) {
        mx = qv[0];
        for (int j = 1; j < A; ++j) mx = qv[j] > mx ? qv[j] : mx;  // jnp.max
    }
    __syncthreads();
    // the online net on obs
    for (int i = tid; i < P.in; i += nt) row[i] = dq_input(a, a.r_obs, s, i);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        cl::cl_forward(P, l, a.online, row);
        __syncthreads();
    }
    if (tid == 0) {  // the TD error, weighted: d loss / d q[a_b] = w 2 (q - td) / B
        float* dq = row + P.l[L - 1].delta;
        const int act = a.r_act[s];
        const float rew = a.r_rew[s];
        const float notdone = a.r_done[s] ? 0.0f : 1.0f;
        const float td = rew + (a.gamma * mx) * notdone;
        const bool ok = act >= 0 && act < A;  // (an action outside [0, A) adds nothing)
        const float d = (ok ? dq[act] : td) - td;
        const float w = p.weights[b];
        a.scratch[P.sq_off + b] = w * (d * d);
        const float g = w * ((d + d) / (float)batch);
        for (int j = 0; j < A; ++j) dq[j] = (ok && j == act) ? g : 0.0f;
        p.absd[b] = __builtin_fabsf(d);
        p.leaves[s] = 0.0f;  // (the priority kernel's integer max starts from 0.0; every row of the slot stores it)
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
        cl::cl_backward(P, l, a.online, row);
        __syncthreads();
    }
    float* dst = a.scratch + P.rows_off + (int64_t)b * P.row_words;
    for (int i = tid; i < P.row_words; i += nt) dst[i] = row[i];
}

}  // namespace

}  // namespace cper
}  // namespace drl
