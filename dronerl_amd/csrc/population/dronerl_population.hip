// dronerl_population.hip — a population of dense DQN agents ("members") acting and learning in the same
// launches (include/dronerl.h drl_pop_*; the layout in dronerl_population_layout.h).  Every member is one
// train_jax.py:38-115 learner block on its own envs, with oracle/dqn_learner.py's arithmetic bit for bit; the
// member is one more grid dimension, so a step's launch count does not depend on the population's size:
//   drl_pop_act_kernel         Q of every env by its member's online f32 parameters, the epsilon-greedy epilogue
//                              of dronerl_act_common.h with the member's device epsilon, the synthetic columns;
//   drl_pop_replay_add_kernel  env g's drone-0 transition into ring g / E (ReplayBuffer.add_many's slot rule);
//   drl_pop_rows / forward / td / backward / update / counters _kernel
//                              the large-batch learner's chain (largelearn/dronerl_largelearn_chain.h: the same
//                              bodies the single-agent kernels run), a member per grid slice.  A member trains
//                              iff size >= its batch, decided here on the device from its hyperparameter record;
//                              rows at or beyond its batch do nothing; one that does not train still blends its
//                              target when due, decays epsilon and advances its step.  The prioritized
//                              population (perpop/) has rows and TD kernels of its own and launches this
//                              unit's forward, backward, update and counters kernels (launch_pop_*).
// No workgroup waits for another, no float atomic is used, nothing reads host hyperparameters: a step is
// graph-capturable.  Every loop bound comes from the validated plan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "../largelearn/dronerl_largelearn_chain.h"
#include "dronerl_population_layout.h"
#include "dronerl_population_member.h"  // a member's view (shared with perpop/dronerl_perpop.hip)

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {
namespace pop {

namespace {

using ll::ll_f4;

// what dq_input reads of its argument block
struct CodeRows {
    int64_t row_words;
    int32_t code_w;
};

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

}  // namespace

// The counters and Adam's moments of every member from zero, epsilon = the record's eps_start.
__global__ void __launch_bounds__(kThreads) drl_pop_init_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int m = blockIdx.y;
    uint8_t* blk = a.base + a.stride * m;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float* mv = reinterpret_cast<float*>(blk + a.P.pub.m_off);  // (the two moment sets are adjacent)
    if (i < 2 * a.P.n_params) mv[i] = 0.0f;
    if (i == 0) {
        DqnCounters c = {};
        c.epsilon = hrec(a.base, a.hp_off, m).eps_start;
        c.beta1_pow = 1.0;
        c.beta2_pow = 1.0;
        *reinterpret_cast<DqnCounters*>(blk + a.P.pub.counters_off) = c;
    }
}

// The act: workgroup (blockIdx.x, blockIdx.y) takes envs [kActEnvs * x, ...) of member y.  The envs' inputs are
// decoded from the policy code into LDS (dq_input: the learner's decode); then layer by layer thread j computes
// unit j of every env of the tile, kActGroup envs at a time: the env's activations are read from LDS at
// wave-uniform addresses (a broadcast), the unit's weight row from the member's f32 online set.  The sums are
// the learner's (four partial sums over k mod 4, (s0 + s1) + (s2 + s3), + bias), so Q equals oracle.forward bit
// for bit.  Activations pass between layers through two LDS buffers.
__global__ void __launch_bounds__(kActThreads) drl_pop_act_kernel(ActArgs args) {
    (void)args;
    const ActArgs& a = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const ll::Plan& P = a.P;
    extern __shared__ __attribute__((aligned(16))) float pop_lds[];
    const int tid = threadIdx.x, m = blockIdx.y;
    const int64_t e0 = (int64_t)blockIdx.x * kActEnvs;
    const int ne = (int)min((int64_t)kActEnvs, a.E - e0);
    const int64_t g0 = (int64_t)m * a.E + e0;  // the tile's first env in the batch
    const int ldx = a.ldx, ldh = a.ldh;
    float* X = pop_lds;
    float* Hb = X + kActEnvs * ldx;  // two buffers of kActEnvs * ldh floats: layer l writes buffer l & 1
    const uint8_t* blk = a.base + a.stride * m;
    const float* online = reinterpret_cast<const float*>(blk + P.pub.online_off);
    const CodeRows cr = {a.row_words, P.code_w};
    const int in4 = P.in4;
    for (int e = tid; e < ne * in4; e += kActThreads) {
        const int r = e / in4, k = e - r * in4;
        X[r * ldx + k] = k < P.in[0] ? dq_input(cr, a.code, g0 + r, k) : 0.0f;
    }
    __syncthreads();
    const int L = P.n_layers;
    for (int l = 0; l < L; ++l) {
        const int K = P.in[l], J = P.out[l];
        const float* in = l == 0 ? X : Hb + ((l - 1) & 1) * kActEnvs * ldh;
        const int ldi = l == 0 ? ldx : ldh;
        float* out = Hb + (l & 1) * kActEnvs * ldh;
        if (tid < J) {
            const float* w = online + P.woff[l] + (int64_t)tid * K;
            const float bias = online[P.boff[l] + tid];
            const bool hidden = l + 1 < L;
            const int full = K >> 2, t = K & 3;
            for (int r0 = 0; r0 < ne; r0 += kActGroup) {
                int off[kActGroup];
#pragma unroll
                for (int g = 0; g < kActGroup; ++g) off[g] = min(r0 + g, ne - 1) * ldi;  // (a row past the tile repeats the last)
                float s[4][kActGroup];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int g = 0; g < kActGroup; ++g) s[c][g] = 0.0f;
                for (int q = 0; q < full; ++q) {
                    const float w0 = w[4 * q], w1 = w[4 * q + 1], w2 = w[4 * q + 2], w3 = w[4 * q + 3];
#pragma unroll
                    for (int g = 0; g < kActGroup; ++g) {
                        const ll_f4 x = *reinterpret_cast<const ll_f4*>(in + off[g] + 4 * q);
                        s[0][g] = s[0][g] + x.x * w0;
                        s[1][g] = s[1][g] + x.y * w1;
                        s[2][g] = s[2][g] + x.z * w2;
                        s[3][g] = s[3][g] + x.w * w3;
                    }
                }
                if (t) {
                    const float w0 = w[4 * full], w1 = t > 1 ? w[4 * full + 1] : 0.0f, w2 = t > 2 ? w[4 * full + 2] : 0.0f;
#pragma unroll
                    for (int g = 0; g < kActGroup; ++g) {
                        const ll_f4 x = *reinterpret_cast<const ll_f4*>(in + off[g] + 4 * full);
                        s[0][g] = s[0][g] + x.x * w0;
                        if (t > 1) s[1][g] = s[1][g] + x.y * w1;
                        if (t > 2) s[2][g] = s[2][g] + x.z * w2;
                    }
                }
#pragma unroll
                for (int g = 0; g < kActGroup; ++g) {
                    if (r0 + g >= ne) break;
                    const float v = ((s[0][g] + s[1][g]) + (s[2][g] + s[3][g])) + bias;
                    out[(r0 + g) * ldh + tid] = hidden ? (v > 0.0f ? v : 0.0f) : v;
                }
            }
        }
        __syncthreads();
    }
    const float* Q = Hb + ((L - 1) & 1) * kActEnvs * ldh;
    const int NA = P.out[L - 1];
    if (tid < ne) {
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = i < NA ? Q[tid * ldh + i] : 0.0f;
        Epilogue ep;
        ep.seed = a.seed;
        ep.step = a.step;
        ep.env_offset = a.env_offset;
        ep.eps_ptr = a.greedy ? nullptr : &reinterpret_cast<const DqnCounters*>(blk + P.pub.counters_off)->epsilon;
        ep.epsilon = 0.0f;  // (the greedy flag: nothing explores, whatever the member's epsilon)
        ep.actions = a.actions;
        ep.action_stride = a.n_drones;
        ep.q = a.q;
        act_epilogue(ep, g0 + tid, q, NA, true);
    }
    // drones 1..N-1: drl_synth_actions' columns of the tile's envs
    const int nd = a.n_drones - 1;
    for (int e = tid; e < ne * nd; e += kActThreads) {
        const int r = e / nd, d = 1 + (e - r * nd);
        const int64_t env = g0 + r;
        a.actions[env * a.n_drones + d] = synth_action(a.synth_seed, a.synth_step, (uint64_t)(a.env_offset + env), (uint64_t)d);
    }
}

// ReplayBuffer.add_many for every member at once: env g = m * E + i lands in slot (cursor + i) % capacity of
// ring m; with E > capacity the last `capacity` envs of a member are kept (what a sequential add() loop leaves).
// A thread per (env, row word); word 0's thread also stores the action, reward and done.
__global__ void __launch_bounds__(kThreads) drl_pop_replay_add_kernel(AddArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.total * a.row_words) return;
    const int64_t g = e / a.row_words, w = e - g * a.row_words;
    const int64_t m = g / a.E, i = g - m * a.E;
    if (i < a.E - a.capacity) return;
    const int64_t slot = m * a.capacity + (a.cursor + i) % a.capacity;
    a.r_obs[slot * a.row_words + w] = a.code_prev[e];
    a.r_next[slot * a.row_words + w] = a.code[e];
    if (w == 0) {
        a.r_act[slot] = a.actions[g * a.n_drones];
        a.r_rew[slot] = a.rewards[g * a.n_drones];
        a.r_done[slot] = a.dones[g * a.n_drones];
    }
}

// ---- the learner: the large-batch chain with the member in the grid ------------------------------------------
// 1. rows: grid (elements of 2 x max_batch x in4, members)
__global__ void __launch_bounds__(kThreads) drl_pop_rows_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Member v = member_of(a, blockIdx.y);
    if (a.size < v.batch) return;
    ll::rows_body(a.P, v, UniformRows{}, v.batch, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// 2. layer l's forward: grid (row tiles, 2 nets x members, unit tiles)
__global__ void __launch_bounds__(ll::kTileThreads) drl_pop_forward_kernel(PopArgs args, int l) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    const Member v = member_of(a, blockIdx.y >> 1);
    if (a.size < v.batch || (int)blockIdx.x * ll::kTileRows >= v.batch) return;  // (uniform over the workgroup)
    ll::forward_body(a.P, v, v.batch, l, (int)(blockIdx.y & 1), (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 3. TD: grid (max_batch rows, members); the head's deltas divide by the member's batch
__global__ void __launch_bounds__(kThreads) drl_pop_td_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Member v = member_of(a, blockIdx.y);
    if (a.size < v.batch) return;
    ll::td_body(a.P, v, UniformRows{}, v.batch, (int)(blockIdx.x * kThreads + threadIdx.x));
}

// 4. layer l's backward (l >= 1): grid (row tiles, members, unit tiles)
__global__ void __launch_bounds__(ll::kTileThreads) drl_pop_backward_kernel(PopArgs args, int l) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[ll::kTileRows * ll::kChunkStride];
    const Member v = member_of(a, blockIdx.y);
    if (a.size < v.batch || (int)blockIdx.x * ll::kTileRows >= v.batch) return;
    ll::backward_body(a.P, v, v.batch, l, (int)blockIdx.x, (int)blockIdx.z, Xs);
}

// 5. update: grid (column tiles, unit tiles, layers x members).  A member that does not train blends its target
// when due: each thread the two parameters it would have updated (the tiles cover every parameter once).
__global__ void __launch_bounds__(ll::kUpdateThreads) drl_pop_update_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const ll::Plan& P = a.P;
    __shared__ __attribute__((aligned(16))) float Xs[ll::kUpdateChunk * ll::kUpdateCols];
    __shared__ __attribute__((aligned(16))) float Ds[ll::kUpdateChunk * ll::kUpdateUnits];
    const int L = P.n_layers;
    const int m = blockIdx.z / L, l = blockIdx.z - m * L;
    const Member v = member_of(a, m);
    if (a.size >= v.batch) {
        ll::update_body(P, v, v.batch, l, (int)blockIdx.x, (int)blockIdx.y, Xs, Ds);
        return;
    }
    const int k = blockIdx.x * ll::kUpdateCols + (threadIdx.x & (ll::kUpdateCols - 1));
    const int j = blockIdx.y * ll::kUpdateUnits + 2 * (threadIdx.x / ll::kUpdateCols);
    for (int u = 0; u < 2; ++u) {
        const int64_t i = ll::update_param(P, l, j + u, k);
        if (i >= 0) ll::blend_body(v, i);
    }
}

// 6. counters: a workgroup per member
__global__ void __launch_bounds__(kThreads) drl_pop_counters_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float sq[ll::kMaxBatch];
    const Member v = member_of(a, blockIdx.x);
    ll::counters_body(a.P, v, v.batch, a.size >= v.batch ? 1 : 0, sq);
}

// The replay slots each member's next train step samples: slots[m][b] for b < the member's batch, -1 beyond.
__global__ void __launch_bounds__(kThreads) drl_pop_sample_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int m = blockIdx.y, b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= a.P.batch) return;
    const HRec& h = hrec(a.base, a.hp_off, m);
    const DqnCounters* c = reinterpret_cast<const DqnCounters*>(a.base + a.stride * m + a.P.pub.counters_off);
    a.slots[(int64_t)m * a.P.batch + b] = b < h.batch ? dq_sample(h.seed, c->step, b, a.size) : -1;
}

int launch_pop_init(const PopArgs& a, hipStream_t s) {
    const unsigned gx = (unsigned)((2 * a.P.n_params + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(drl_pop_init_kernel, dim3(gx, (unsigned)a.members), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

int launch_pop_act(const ActArgs& a, int lds_bytes, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.E + kActEnvs - 1) / kActEnvs);
    hipLaunchKernelGGL(drl_pop_act_kernel, dim3(tiles, (unsigned)a.members), dim3(kActThreads), (size_t)lds_bytes, s, a);
    return (int)hipGetLastError();
}

int launch_pop_add(const AddArgs& a, hipStream_t s) {
    const int64_t n = a.total * a.row_words;
    hipLaunchKernelGGL(drl_pop_replay_add_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

// ---- the chain's segments: the launches the prioritized population's chain (perpop/dronerl_perpop.hip) takes
// over as they are.  The grid arithmetic lives here alone; the caller reads hipGetLastError behind its last launch.
// 1. the rows (uniform draws)
void launch_pop_rows(const PopArgs& a, hipStream_t s) {
    const int64_t elems = 2 * (int64_t)a.P.batch * a.P.in4;
    hipLaunchKernelGGL(drl_pop_rows_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads), (unsigned)a.members),
                       dim3(kThreads), 0, s, a);
}

// 2. every layer's forward
void launch_pop_forward(const PopArgs& a, hipStream_t s) {
    const ll::Plan& P = a.P;
    const unsigned M = (unsigned)a.members;
    for (int l = 0; l < P.n_layers; ++l)
        hipLaunchKernelGGL(drl_pop_forward_kernel, dim3((unsigned)ll::row_tiles(P), 2 * M, (unsigned)ll::unit_tiles(P.out[l])),
                           dim3(ll::kTileThreads), 0, s, a, l);
}

// 4.-5. the backward pass of every layer >= 1, then the update
void launch_pop_backward_update(const PopArgs& a, hipStream_t s) {
    const ll::Plan& P = a.P;
    const unsigned M = (unsigned)a.members;
    const int L = P.n_layers;
    for (int l = L - 1; l >= 1; --l)
        hipLaunchKernelGGL(drl_pop_backward_kernel, dim3((unsigned)ll::row_tiles(P), M, (unsigned)ll::unit_tiles(P.in[l])),
                           dim3(ll::kTileThreads), 0, s, a, l);
    int kt = 0, jt = 0;  // (the widest layer's tiles; a workgroup outside its layer's returns at once)
    for (int l = 0; l < L; ++l) {
        kt = ll::update_col_tiles(P, l) > kt ? ll::update_col_tiles(P, l) : kt;
        jt = ll::update_unit_tiles(P, l) > jt ? ll::update_unit_tiles(P, l) : jt;
    }
    hipLaunchKernelGGL(drl_pop_update_kernel, dim3((unsigned)kt, (unsigned)jt, (unsigned)L * M), dim3(ll::kUpdateThreads),
                       0, s, a);
}

// 6. the counters
void launch_pop_counters(const PopArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_pop_counters_kernel, dim3((unsigned)a.members), dim3(kThreads), 0, s, a);
}

int launch_pop_train(const PopArgs& a, hipStream_t s) {
    const ll::Plan& P = a.P;
    const unsigned M = (unsigned)a.members;
    launch_pop_rows(a, s);
    launch_pop_forward(a, s);
    hipLaunchKernelGGL(drl_pop_td_kernel, dim3((unsigned)((P.batch + kThreads - 1) / kThreads), M), dim3(kThreads), 0, s, a);
    launch_pop_backward_update(a, s);
    launch_pop_counters(a, s);
    return (int)hipGetLastError();
}

int launch_pop_sample(const PopArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_pop_sample_kernel, dim3((unsigned)((a.P.batch + kThreads - 1) / kThreads), (unsigned)a.members),
                       dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace pop
}  // namespace drl
