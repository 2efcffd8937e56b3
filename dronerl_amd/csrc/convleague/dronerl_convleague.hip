// dronerl_convleague.hip — the act of a league of conv DQN learners that share their envs (include/dronerl.h
// drl_convleague_*; the plan in dronerl_convleague_layout.h).  Learner k is member k of a conv population block
// and drives drone index k of every env:
//   drl_convleague_act_kernel   workgroup (tile x, learner y) takes T envs of learner y through every layer on
//                               block y of drl_obs_code_all's output, then the epsilon-greedy epilogue of
//                               dronerl_act_common.h with the learner's device epsilon and the stream seed + y,
//                               into column y.
// drl_convpop_act's workgroup takes one env and fetches every weight once per product; here a weight word fetched
// from L2 serves the tile's T envs.  The arithmetic of an env is cl::cl_forward's (convlearn/
// dronerl_convlearn_rows.h) bit for bit: a conv output sums its taps in (ci, ky, kx) order from 0.0, taps outside
// the map skipped, then + bias; a dense unit's lane c sums k = c (mod 64) in k order, then the xor tree at
// distances 1, 2, .., 32, then + bias; relu everywhere but the head; every product and sum rounded on its own.
// The tiling decides which thread does a sum, never its order.  No workgroup waits for another, no float atomic
// is used, nothing is allocated: the call is graph-capturable.  Every loop bound is the validated plan's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "dronerl_convleague_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the learners
#pragma clang fp contract(off)

// cvl::tile_forward and its helpers (shared with convselfplay/dronerl_convselfplay.hip)
#include "dronerl_convleague_tile.h"

namespace drl {
namespace cvl {

// Workgroup (blockIdx.x, blockIdx.y) takes envs [T * x, T * x + T) of learner y.
template <int T>
__global__ void __launch_bounds__(kThreadsMax) drl_convleague_act_kernel(ActArgs args) {
    (void)args;
    const ActArgs& a = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::Plan& P = a.P;
    const ActPlan& A = a.A;
    extern __shared__ float4 cvl_lds4[];
    float* rows = reinterpret_cast<float*>(cvl_lds4);
    const int tid = threadIdx.x, nt = blockDim.x, m = blockIdx.y, S = A.row_words;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int ne = (int)min((int64_t)T, a.E - e0);
    const uint8_t* blk = a.base + a.stride * m;
    const float* online = reinterpret_cast<const float*>(blk + P.pub.online_off);
    // The tile's code rows (contiguous in block m): a thread reads a cell's u16 once (consecutive threads,
    // consecutive cells) and decodes its six channels as the learner does (dq_input); rows past E hold 0.0.
    {
        const CodeRows cr = {a.row_words, P.code_w};
        const uint32_t* src = a.codes + ((int64_t)m * a.E + e0) * a.row_words;
        const int cells = P.in / 6;
        for (int i = tid; i < T * cells; i += nt) {
            const int r = i / cells, cl_ = i - r * cells;
            float* xr = rows + r * S + 6 * cl_;
#pragma unroll
            for (int ch = 0; ch < 6; ++ch) xr[ch] = r < ne ? dq_input(cr, src, r, 6 * cl_ + ch) : 0.0f;
        }
    }
    __syncthreads();
    const int L = P.n_layers;
    for (int l = 0; l < L; ++l) {
        tile_forward<T>(P, A, l, online, rows);
        __syncthreads();
    }
    const int NA = P.n_actions;
    if (tid < ne) {
        const float* Q = rows + tid * S + A.out[L - 1];
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = i < NA ? Q[i] : 0.0f;
        Epilogue ep;
        ep.seed = a.seed + (uint64_t)m;  // learner k's exploration stream
        ep.step = a.step;
        ep.env_offset = a.env_offset;
        ep.eps_ptr = a.greedy ? nullptr : &reinterpret_cast<const DqnCounters*>(blk + P.pub.counters_off)->epsilon;
        ep.epsilon = 0.0f;  // (the greedy flag: nothing explores, whatever the learner's epsilon)
        ep.actions = a.actions + m;  // column m of [E][n_drones]
        ep.action_stride = a.n_drones;
        ep.q = a.q ? a.q + (int64_t)m * a.E * NA : nullptr;
        act_epilogue(ep, e0 + tid, q, NA, true);
    }
}

namespace {

template <int T>
int launch_tile(const ActArgs& a, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.E + T - 1) / T);
    if (a.A.lds_bytes > 64 * 1024) {  // (host-side, no stream work: the larger rows' plan needs the opt-in)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(drl_convleague_act_kernel<T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(drl_convleague_act_kernel<T>, dim3(tiles, (unsigned)a.members), dim3((unsigned)a.A.threads),
                       (size_t)a.A.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_convleague_act(const ActArgs& a, hipStream_t s) {
    switch (a.A.env_tile) {
        case 16: return launch_tile<16>(a, s);
        case 8: return launch_tile<8>(a, s);
        case 4: return launch_tile<4>(a, s);
        case 2: return launch_tile<2>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace cvl
}  // namespace drl
