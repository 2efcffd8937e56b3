// dronerl_league.hip — a league of DQN learners that share their envs (include/dronerl.h drl_league_*; the plan
// in dronerl_league_layout.h).  Learner k is member k of a population block and drives drone index k of every
// env:
//   drl_league_act_kernel         Q of every env by each learner's online f32 parameters on block k of
//                                 drl_obs_code_all's output, the epsilon-greedy epilogue of dronerl_act_common.h
//                                 with the learner's device epsilon and the stream seed + k, into column k;
//   drl_league_replay_add_kernel  env i's drone-k transition into slot (cursor + i) % capacity of ring k.
// The sums are the learner's (four partial sums over k mod 4, (s0 + s1) + (s2 + s3), + bias; every product and
// sum rounded on its own), so Q equals oracle.forward bit for bit: the tiling decides which thread does a sum,
// never its order.  No workgroup waits for another, no float atomic is used, nothing is allocated.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "dronerl_league_layout.h"

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {
namespace league {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));  // two partial sums side by side (packed f32 multiply, add)
typedef float f4 __attribute__((ext_vector_type(4)));

// what the act epilogue reads of its argument block (dronerl_act_common.h)
struct Epilogue {
    uint64_t seed, step;
    int64_t env_offset;
    const float* eps_ptr;
    float epsilon;
    int32_t* actions;
    int64_t action_stride;
    float* q;
};

// One cell of a policy-code row as its six observation channels (dq_input's rules, a cell at a time).
__device__ __forceinline__ void decode_cell(uint32_t h, float* __restrict__ o) {
    const uint32_t obj = h & 7u, air = h >> 3;
    o[0] = air ? 1.0f : 0.0f;
    o[1] = (obj == OBJ_PACKET || (air & 0x80u)) ? 1.0f : 0.0f;
    o[2] = obj == OBJ_DROPZONE ? 1.0f : 0.0f;
    o[3] = obj == OBJ_STATION ? 1.0f : 0.0f;
    o[4] = air ? (float)((int)(air & 0x7fu) - 1) / 100.0f : 0.0f;
    o[5] = obj == OBJ_SKYSCRAPER ? 1.0f : 0.0f;
}

}  // namespace

// Workgroup (blockIdx.x, blockIdx.y) takes envs [kEnvTile * x, ...) of learner y.  Lane (env, half) of wave w
// holds units lane_unit(w, half) .. + kUnitsPerLane - 1 of the pass at hand for its env.  The flattened sequence
// (layer, pass, chunk) is walked once; the next chunk's weights are fetched into registers before the current
// chunk's arithmetic and stored to LDS after it, so the loads' latency is covered.
__global__ void __launch_bounds__(kActThreads) drl_league_act_kernel(ActArgs args) {
    (void)args;
    const ActArgs& a = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const ll::Plan& P = a.P;
    extern __shared__ __attribute__((aligned(16))) float league_lds[];
    const int tid = threadIdx.x, m = blockIdx.y;
    const int lane = tid & 63, wave = tid >> 6, er = lane & (kEnvTile - 1), half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kEnvTile;
    const int ne = (int)min((int64_t)kEnvTile, a.E - e0);
    const int ldx = a.A.ldx, lda = a.A.lda;
    float* RA = league_lds;
    float* RB = RA + a.A.a_floats;
    float* Ws = RB + a.A.b_floats;
    const uint8_t* blk = a.base + a.stride * m;
    const float* online = reinterpret_cast<const float*>(blk + P.pub.online_off);

    const int L = P.n_layers;
    float pre[kStageLoads];
    auto fetch = [&](int l, int p, int c) {
        const int K = P.in[l], J = P.out[l];
        const float* w = online + P.woff[l];
        const int k = c * kChunkK + stage_k(tid);
#pragma unroll
        for (int i = 0; i < kStageLoads; ++i) {
            const int j = p * kPassUnits + stage_unit(tid, i);
            pre[i] = (j < J && k < K) ? w[(int64_t)j * K + k] : 0.0f;
        }
    };
    const int row = min(er, ne - 1);  // (a lane past the tile repeats the last env and stores nothing)
    const int ub = lane_unit(wave, half);
    f2 s01[kUnitsPerLane], s23[kUnitsPerLane];
    int l = 0, p = 0, c = 0;
    fetch(0, 0, 0);
    // the tile's code rows (contiguous in block m), read once into the staging area, then decoded cell by cell as
    // the learner decodes its rows; the pad columns hold 0.0
    {
        const int rw = (int)a.row_words, W = P.code_w, cells = W * W;
        const int cpg = lay::code_cpg(W), cpg8 = lay::code_cpg8(W);
        uint32_t* raw = reinterpret_cast<uint32_t*>(Ws);
        const uint32_t* src = a.codes + ((int64_t)m * a.E + e0) * rw;
        for (int e = tid; e < ne * rw; e += kActThreads) raw[e] = src[e];
        __syncthreads();
        const uint16_t* raw16 = reinterpret_cast<const uint16_t*>(raw);
        for (int e = tid; e < ne * cells; e += kActThreads) {
            const int r = e / cells, cl = e - r * cells, grp = cl / cpg;
            decode_cell(raw16[r * rw * 2 + grp * cpg8 + (cl - grp * cpg)], RA + r * ldx + 6 * cl);
        }
        const int pad = P.in4 - P.in[0];
        for (int e = tid; e < ne * pad; e += kActThreads) RA[(e / pad) * ldx + P.in[0] + e % pad] = 0.0f;
    }
    while (l < L) {
        const int K = P.in[l], J = P.out[l];
        const int nch = chunk_count(K), npass = pass_count(J);
        __syncthreads();  // the chunk before this one has been read (at first: the code rows; the inputs are written)
#pragma unroll
        for (int i = 0; i < kStageLoads; ++i) Ws[stage_unit(tid, i) * kChunkK + stage_k(tid)] = pre[i];
        __syncthreads();
        int nl = l, np = p, nc = c + 1;
        if (nc == nch) {
            nc = 0;
            if (++np == npass) {
                np = 0;
                ++nl;
            }
        }
        if (nl < L) fetch(nl, np, nc);
        if (c == 0) {
#pragma unroll
            for (int u = 0; u < kUnitsPerLane; ++u) s01[u] = s23[u] = f2{0.0f, 0.0f};
        }
        if (p * kPassUnits + lane_unit(wave, 0) < J) {  // (uniform over the wave)
            const float* in = (l & 1) ? RB : RA;
            const float* xr = in + row * (l == 0 ? ldx : lda) + c * kChunkK;
            const float* wr = Ws + ub * kChunkK;
            const int nq = chunk_quads(K, c);
            // Two register sets take turns: the next 4-column step's operands are read while this one's products
            // are summed (a chunk has an even number of steps: chunk_quads).
            auto load = [&](int q, f4& x, f4 (&w)[kUnitsPerLane]) {
                x = *reinterpret_cast<const f4*>(xr + 4 * q);
#pragma unroll
                for (int u = 0; u < kUnitsPerLane; ++u) w[u] = *reinterpret_cast<const f4*>(wr + u * kChunkK + 4 * q);
            };
            auto mac = [&](const f4& x, const f4 (&w)[kUnitsPerLane]) {
                const f2 x01 = {x.x, x.y}, x23 = {x.z, x.w};
#pragma unroll
                for (int u = 0; u < kUnitsPerLane; ++u) {
                    const f2 w01 = {w[u].x, w[u].y}, w23 = {w[u].z, w[u].w};
                    s01[u] = s01[u] + x01 * w01;
                    s23[u] = s23[u] + x23 * w23;
                }
            };
            f4 xa, xb, wa[kUnitsPerLane], wb[kUnitsPerLane];
            load(0, xa, wa);
            for (int q = 0; q < nq; q += 2) {
                load(q + 1, xb, wb);
                __builtin_amdgcn_sched_barrier(0);
                mac(xa, wa);
                __builtin_amdgcn_sched_barrier(0);
                load(q + 2 < nq ? q + 2 : q, xa, wa);
                __builtin_amdgcn_sched_barrier(0);
                mac(xb, wb);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (c == nch - 1) {
                float* out = (l & 1) ? RA : RB;
                const bool hidden = l + 1 < L;
                const int jb = p * kPassUnits + ub;
                float v[kUnitsPerLane];
#pragma unroll
                for (int u = 0; u < kUnitsPerLane; ++u) {
                    const float bias = jb + u < J ? online[P.boff[l] + jb + u] : 0.0f;
                    const float z = ((s01[u].x + s01[u].y) + (s23[u].x + s23[u].y)) + bias;
                    v[u] = hidden ? (z > 0.0f ? z : 0.0f) : z;
                }
                if (er < ne) {
#pragma unroll
                    for (int u = 0; u < kUnitsPerLane; u += 4)
                        if (jb + u < J) *reinterpret_cast<f4*>(out + er * lda + jb + u) = f4{v[u], v[u + 1], v[u + 2], v[u + 3]};
                }
            }
        }
        l = nl;
        p = np;
        c = nc;
    }
    __syncthreads();
    const float* Q = ((L - 1) & 1) ? RA : RB;
    const int NA = P.out[L - 1];
    if (tid < ne) {
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = i < NA ? Q[tid * lda + i] : 0.0f;
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

// ReplayBuffer.add_many for every learner at once: env i's drone-k transition lands in slot (cursor + i) %
// capacity of ring k; with E > capacity the last `capacity` envs are kept.  A thread per (learner, env, row
// word); word 0's thread also stores the action, reward and done of column k.
__global__ void __launch_bounds__(kThreads) drl_league_replay_add_kernel(AddArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.total * a.row_words) return;
    const int64_t g = e / a.row_words, w = e - g * a.row_words;
    const int64_t k = g / a.E, i = g - k * a.E;
    if (i < a.E - a.capacity) return;
    const int64_t slot = k * a.capacity + (a.cursor + i) % a.capacity;
    a.r_obs[slot * a.row_words + w] = a.codes_prev[e];
    a.r_next[slot * a.row_words + w] = a.codes[e];
    if (w == 0) {
        a.r_act[slot] = a.actions[i * a.n_drones + k];
        a.r_rew[slot] = a.rewards[i * a.n_drones + k];
        a.r_done[slot] = a.dones[i * a.n_drones + k];
    }
}

int launch_league_act(const ActArgs& a, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.E + kEnvTile - 1) / kEnvTile);
    if (a.A.lds_bytes > 64 * 1024) {  // (host-side, no stream work: the widest nets' plan needs the opt-in)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(drl_league_act_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(drl_league_act_kernel, dim3(tiles, (unsigned)a.members), dim3(kActThreads), (size_t)a.A.lds_bytes, s, a);
    return (int)hipGetLastError();
}

int launch_league_add(const AddArgs& a, hipStream_t s) {
    const int64_t n = a.total * a.row_words;
    hipLaunchKernelGGL(drl_league_replay_add_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace league
}  // namespace drl
