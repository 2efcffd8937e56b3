// dronerl_convselfplay.hip — the act of shared-policy self-play with conv learners (include/dronerl.h
// drl_convselfplay_act; the row map in dronerl_convselfplay_layout.h, the plan in convleague/
// dronerl_convleague_layout.h).  Learner k is member k of a conv population block and drives drone indices
// drones[k][0 .. team - 1] of every env; its rows are the team * E (drone, env) pairs flattened slot-major,
// r = j * E + i:
//   drl_convselfplay_act_kernel   workgroup (tile x, learner y) takes T consecutive rows of learner y through
//                                 every layer, each row gathered from codes[drones[y][j]][i], then the
//                                 epsilon-greedy epilogue of dronerl_act_common.h with the learner's device
//                                 epsilon and the stream seed + drone index, scattered into that drone's column.
// The tiling and the per-layer arithmetic are the conv league act's (cvl::tile_forward, convleague/
// dronerl_convleague_tile.h): Q of a row is cl::cl_forward's bit for bit and, with a team of one on drone k,
// drl_convleague_act's.  The league's kernel is left as it is: its tile is one drone's envs, read as one contiguous
// block.  No workgroup waits for another, no float atomic is used, nothing is allocated: the call is
// graph-capturable.  Every loop bound is the validated plan's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "dronerl_convselfplay_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the learners
#pragma clang fp contract(off)

#include "../convleague/dronerl_convleague_tile.h"

namespace drl {
namespace cvs {

using cvl::ActPlan;
using cvl::CodeRows;
using cvl::Epilogue;

// Workgroup (blockIdx.x, blockIdx.y) takes rows [T * x, T * x + T) of learner y.
template <int T>
__global__ void __launch_bounds__(cvl::kThreadsMax) drl_convselfplay_act_kernel(ActArgs args) {
    (void)args;
    const ActArgs& sa = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cvl::ActArgs& a = sa.c;
    const cl::Plan& P = a.P;
    const ActPlan& A = a.A;
    extern __shared__ float4 cvs_lds4[];
    float* rows = reinterpret_cast<float*>(cvs_lds4);
    const int tid = threadIdx.x, nt = blockDim.x, m = blockIdx.y, S = A.row_words;
    const int64_t r0 = (int64_t)blockIdx.x * T;
    const int ne = tile_rows(r0, T, sa.rows);
    const uint8_t* blk = a.base + a.stride * m;
    const float* online = reinterpret_cast<const float*>(blk + P.pub.online_off);
    const uint8_t* team = sa.drones + m * sa.team;
    // The tile's code rows: nt / T threads per row (the workgroup is a multiple of 256 threads, T at most 16), so a
    // thread splits its one row into (slot, env) once and then reads that row's cells, a u16 each (consecutive
    // threads, consecutive cells), decoding the six channels as the learner does (dq_input); rows past the
    // learner's hold 0.0.
    {
        const CodeRows cr = {a.row_words, P.code_w};
        const int cells = P.in / 6;
        const int rt = row_threads(nt, T), t = tid / rt;
        float* xr = rows + t * S;
        if (t < ne) {
            const RowPlace p = place_row(team, r0 + t, a.E);
            const uint32_t* src = a.codes + code_row(p, a.E) * a.row_words;
            for (int cl_ = tid - t * rt; cl_ < cells; cl_ += rt) {
#pragma unroll
                for (int ch = 0; ch < 6; ++ch) xr[6 * cl_ + ch] = dq_input(cr, src, 0, 6 * cl_ + ch);
            }
        } else {
            for (int cl_ = tid - t * rt; cl_ < cells; cl_ += rt) {
#pragma unroll
                for (int ch = 0; ch < 6; ++ch) xr[6 * cl_ + ch] = 0.0f;
            }
        }
    }
    __syncthreads();
    const int L = P.n_layers;
    for (int l = 0; l < L; ++l) {
        cvl::tile_forward<T>(P, A, l, online, rows);
        __syncthreads();
    }
    const int NA = P.n_actions;
    if (tid < ne) {
        const float* Q = rows + tid * S + A.out[L - 1];
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = i < NA ? Q[i] : 0.0f;
        const RowPlace p = place_row(team, r0 + tid, a.E);
        Epilogue ep;
        ep.seed = a.seed + (uint64_t)p.dr;  // the drone's exploration stream: two drones of a team never share one
        ep.step = a.step;
        ep.env_offset = a.env_offset;
        ep.eps_ptr = a.greedy ? nullptr : &reinterpret_cast<const DqnCounters*>(blk + P.pub.counters_off)->epsilon;
        ep.epsilon = 0.0f;  // (the greedy flag: nothing explores, whatever the learner's epsilon)
        ep.actions = a.actions + p.dr;  // column dr of [E][n_drones]: word action_word(p, n_drones) at env p.i
        ep.action_stride = a.n_drones;
        ep.q = a.q ? a.q + q_block(m, sa.team, p, a.E, NA) : nullptr;  // [members][team][E][n_actions]
        act_epilogue(ep, p.i, q, NA, true);
    }
}

namespace {

template <int T>
int launch_tile(const ActArgs& a, hipStream_t s) {
    const unsigned tiles = (unsigned)tile_count(a.rows, T);
    if (a.c.A.lds_bytes > 64 * 1024) {  // (host-side, no stream work: the larger rows' plan needs the opt-in)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(drl_convselfplay_act_kernel<T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, cvl::kLdsLimit);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(drl_convselfplay_act_kernel<T>, dim3(tiles, (unsigned)a.c.members),
                       dim3((unsigned)a.c.A.threads), (size_t)a.c.A.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_convselfplay_act(const ActArgs& a, hipStream_t s) {
    switch (a.c.A.env_tile) {
        case 16: return launch_tile<16>(a, s);
        case 8: return launch_tile<8>(a, s);
        case 4: return launch_tile<4>(a, s);
        case 2: return launch_tile<2>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace cvs
}  // namespace drl
