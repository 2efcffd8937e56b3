// dronerl_selfplay.hip — shared-policy self-play: learners that each drive a team of drones of the shared envs
// (include/dronerl.h drl_selfplay_*; the row map in dronerl_selfplay_layout.h, the plan in
// league/dronerl_league_layout.h).  Learner k is member k of a population block and drives drone indices
// drones[k][0 .. team - 1] of every env; its rows are the team * E (drone, env) pairs flattened slot-major,
// r = j * E + i:
//   drl_selfplay_act_kernel         Q of 32 consecutive rows of one learner by its online f32 parameters, each row
//                                   gathered from codes[drones[k][j]][i]; the epsilon-greedy epilogue of
//                                   dronerl_act_common.h with the learner's device epsilon and the stream seed +
//                                   drone index, scattered into that drone's column;
//   drl_selfplay_replay_add_kernel  row r into slot (cursor + r) % capacity of ring k (add_many's rule on the
//                                   team's rows).
// The tiling, the weight staging and the sums are the league act's (four partial sums over k mod 4, (s0 + s1) +
// (s2 + s3), + bias; every product and sum rounded on its own), so Q equals oracle.forward bit for bit and, with
// a team of one on drone k, drl_league_act's.  The league's kernel is left as it is: its tile is one drone's
// envs, read as one contiguous block, and its timings are pinned.  No workgroup waits for another, no float atomic
// is used, nothing is allocated.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "dronerl_selfplay_layout.h"

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {
namespace selfplay {

using namespace drl::league;  // the plan's constants and index maps (kEnvTile rows of a learner per workgroup)

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

// Workgroup (blockIdx.x, blockIdx.y) takes rows [kEnvTile * x, ...) of learner y.  Lane (row, half) of wave w
// holds units lane_unit(w, half) .. + kUnitsPerLane - 1 of the pass at hand for its row.  The flattened sequence
// (layer, pass, chunk) is walked once; the next chunk's weights are fetched into registers before the current
// chunk's arithmetic and stored to LDS after it, so the loads' latency is covered.
__global__ void __launch_bounds__(kActThreads) drl_selfplay_act_kernel(ActArgs args) {
    (void)args;
    const ActArgs& a = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const ll::Plan& P = a.P;
    extern __shared__ __attribute__((aligned(16))) float selfplay_lds[];
    const int tid = threadIdx.x, m = blockIdx.y;
    const int lane = tid & 63, wave = tid >> 6, er = lane & (kEnvTile - 1), half = lane >> 5;
    const int r0 = (int)blockIdx.x * kEnvTile;  // (rows < 2^31: checked by the host)
    const int ne = min(kEnvTile, a.rows - r0);
    const int E = (int)a.E;
    const int ldx = a.A.ldx, lda = a.A.lda;
    float* RA = selfplay_lds;
    float* RB = RA + a.A.a_floats;
    float* Ws = RB + a.A.b_floats;
    const uint8_t* blk = a.base + a.stride * m;
    const float* online = reinterpret_cast<const float*>(blk + P.pub.online_off);
    const uint8_t* team = a.drones + m * a.team;

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
    const int row = min(er, ne - 1);  // (a lane past the tile repeats the last row and stores nothing)
    const int ub = lane_unit(wave, half);
    f2 s01[kUnitsPerLane], s23[kUnitsPerLane];
    int l = 0, p = 0, c = 0;
    fetch(0, 0, 0);
    // the tile's code rows (row r0 + t from codes[drones[m][j]][i], each contiguous), read once into the staging
    // area, then decoded cell by cell as the learner decodes its rows; the pad columns hold 0.0
    {
        const int rw = (int)a.row_words, W = P.code_w, cells = W * W;
        const int cpg = lay::code_cpg(W), cpg8 = lay::code_cpg8(W);
        uint32_t* raw = reinterpret_cast<uint32_t*>(Ws);
        // kRowThreads threads per row, 16 bytes each per turn (a row is a multiple of 16 words, 16-byte aligned on
        // both sides): one (slot, env) split per thread
        constexpr int kRowThreads = kActThreads / kEnvTile;
        const int t = tid / kRowThreads;
        if (t < ne) {
            const int r = r0 + t, j = r / E;
            const uint4* src = reinterpret_cast<const uint4*>(a.codes + ((int64_t)team[j] * E + (r - j * E)) * rw);
            uint4* dst = reinterpret_cast<uint4*>(raw + t * rw);
            for (int v = tid % kRowThreads; v < rw / 4; v += kRowThreads) dst[v] = src[v];
        }
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
        const int r = r0 + tid, j = r / E, i = r - j * E, dr = team[j];
        Epilogue ep;
        ep.seed = a.seed + (uint64_t)dr;  // the drone's exploration stream: two drones of a team never share one
        ep.step = a.step;
        ep.env_offset = a.env_offset;
        ep.eps_ptr = a.greedy ? nullptr : &reinterpret_cast<const DqnCounters*>(blk + P.pub.counters_off)->epsilon;
        ep.epsilon = 0.0f;  // (the greedy flag: nothing explores, whatever the learner's epsilon)
        ep.actions = a.actions + dr;  // column dr of [E][n_drones]
        ep.action_stride = a.n_drones;
        ep.q = a.q ? a.q + ((int64_t)m * a.team + j) * E * NA : nullptr;  // [members][team][E][n_actions]
        act_epilogue(ep, i, q, NA, true);
    }
}

// ReplayBuffer.add_many for every learner at once on its team's rows taken slot-major: row r = j * E + i (env
// i's transition of drone drones[k][j]) lands in slot (cursor + r) % capacity of ring k; with team * E > capacity
// the last `capacity` rows are kept.  A thread per (learner, row, row word); word 0's thread also stores the
// action, reward and done of the drone's column.
__global__ void __launch_bounds__(kThreads) drl_selfplay_replay_add_kernel(AddArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.total * a.row_words) return;
    const int64_t g = e / a.row_words, w = e - g * a.row_words;
    const int64_t k = g / a.rows, r = g - k * a.rows;
    if (!row_kept(r, a.rows, a.capacity)) return;
    const RowSource s = row_source(r, a.E);
    const int64_t dr = a.drones[k * a.team + s.j];
    const int64_t slot = k * a.capacity + ring_slot(a.cursor, r, a.capacity);
    const int64_t src = (dr * a.E + s.i) * a.row_words + w;
    a.r_obs[slot * a.row_words + w] = a.codes_prev[src];
    a.r_next[slot * a.row_words + w] = a.codes[src];
    if (w == 0) {
        a.r_act[slot] = a.actions[s.i * a.n_drones + dr];
        a.r_rew[slot] = a.rewards[s.i * a.n_drones + dr];
        a.r_done[slot] = a.dones[s.i * a.n_drones + dr];
    }
}

int launch_selfplay_act(const ActArgs& a, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.rows + kEnvTile - 1) / kEnvTile);
    if (a.A.lds_bytes > 64 * 1024) {  // (host-side, no stream work: the widest nets' plan needs the opt-in)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(drl_selfplay_act_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(drl_selfplay_act_kernel, dim3(tiles, (unsigned)a.members), dim3(kActThreads), (size_t)a.A.lds_bytes, s, a);
    return (int)hipGetLastError();
}

int launch_selfplay_add(const AddArgs& a, hipStream_t s) {
    const int64_t n = a.total * a.row_words;
    hipLaunchKernelGGL(drl_selfplay_replay_add_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace selfplay
}  // namespace drl
