// dronerl_convpop.hip — a population of conv DQN agents ("members") acting and learning in the same launches
// (include/dronerl.h drl_convpop_*; the layout in dronerl_convpop_layout.h).  Every member is one
// train_jax.py:38-115 learner block with network_type == 'conv' on its own envs, with
// drl_convnet_dqn_large_train's arithmetic bit for bit; the member is one more grid dimension, so a step's launch
// count does not depend on the population's size:
//   drl_convpop_act_kernel     one workgroup per env of one member: the policy code decoded into the row's LDS
//                              image (dq_input: the learner's decode), cl::cl_forward layer by layer on the
//                              member's f32 online set -- the device function the rows kernel runs, so the act's Q
//                              is the learner's own Q bit for bit --, the epsilon-greedy epilogue of
//                              dronerl_act_common.h with the member's device epsilon, the synthetic columns.
//                              There is no packed image and nothing is re-packed after a train step.  The MFMA
//                              conv act (drl_convnet_act) agrees with this forward to about 1e-5, not bit for
//                              bit: a member reproduces under the population API, not necessarily under train().
//   drl_convpop_rows / dense_grad / conv_grad / update / counters _kernel
//                              the conv large-batch learner's chain (convlarge/dronerl_convlarge_chain.h: the
//                              same bodies the single-agent kernels run), a member per grid slice.  A member
//                              trains iff size >= its batch, decided here on the device from its hyperparameter
//                              record; rows and chunks at or beyond its batch do nothing and are never read; one
//                              that does not train still blends its target when due, decays epsilon and advances
//                              its step.
// The rings are the dense population's (drl_pop_replay_add).  No workgroup waits for another, no float atomic is
// used, nothing reads host hyperparameters: a step is graph-capturable.  Every loop bound is the validated plan's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "../convlearn/dronerl_convlearn_rows.h"
#include "../convlarge/dronerl_convlarge_chain.h"
#include "../population/dronerl_population_member.h"  // pop::hparams_into: the record's copy into a view
#include "dronerl_convpop_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the other learners
#pragma clang fp contract(off)

namespace drl {
namespace cp {

namespace {

// A member's view: the fields the chain's bodies and dronerl_learn_common.h read (cl::LearnArgs' names).
struct Member {
    int32_t batch, code_w;
    float* online;
    float* target;
    float* adam_m;
    float* adam_v;
    DqnCounters* ctr;
    float* scratch;
    const uint32_t* r_obs;
    const uint32_t* r_next;
    int64_t row_words;
    const int32_t* r_act;
    const float* r_rew;
    const uint8_t* r_done;
    int64_t size;
    uint64_t seed;
    float gamma, b1, b2, c1, c2, adam_eps, neg_lr, tau, one_minus_tau, eps_decay, eps_end;
    double b1d, b2d;
    int32_t target_every, eps_every;
};

__device__ __forceinline__ const HRec& hrec(const uint8_t* base, int64_t hp_off, int m) {
    return *reinterpret_cast<const HRec*>(base + hp_off + kHRecStride * m);
}

__device__ __forceinline__ Member member_of(const PopArgs& a, int m) {
    const cl::Plan& P = a.P;
    uint8_t* blk = a.base + a.stride * m;
    const HRec& h = hrec(a.base, a.hp_off, m);
    Member v;
    v.batch = h.batch;
    v.code_w = P.code_w;
    v.online = reinterpret_cast<float*>(blk + P.pub.online_off);
    v.target = reinterpret_cast<float*>(blk + P.pub.target_off);
    v.adam_m = reinterpret_cast<float*>(blk + P.pub.m_off);
    v.adam_v = reinterpret_cast<float*>(blk + P.pub.v_off);
    v.ctr = reinterpret_cast<DqnCounters*>(blk + P.pub.counters_off);
    v.scratch = reinterpret_cast<float*>(blk + P.pub.scratch_off);
    const int64_t r0 = a.capacity * m;
    v.r_obs = a.r_obs + r0 * a.row_words;
    v.r_next = a.r_next + r0 * a.row_words;
    v.row_words = a.row_words;
    v.r_act = a.r_act + r0;
    v.r_rew = a.r_rew + r0;
    v.r_done = a.r_done + r0;
    v.size = a.size;
    v.seed = h.seed;
    pop::hparams_into(h, v);
    return v;
}

__device__ __forceinline__ int chunks_of(int batch) { return (batch + cg::kChunkRows - 1) / cg::kChunkRows; }

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
__global__ void __launch_bounds__(kThreads) drl_convpop_init_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int m = blockIdx.y;
    uint8_t* blk = a.base + a.stride * m;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.P.n_params) {
        reinterpret_cast<float*>(blk + a.P.pub.m_off)[i] = 0.0f;
        reinterpret_cast<float*>(blk + a.P.pub.v_off)[i] = 0.0f;
    }
    if (i == 0) {
        DqnCounters c = {};
        c.epsilon = hrec(a.base, a.hp_off, m).eps_start;
        c.beta1_pow = 1.0;
        c.beta2_pow = 1.0;
        *reinterpret_cast<DqnCounters*>(blk + a.P.pub.counters_off) = c;
    }
}

// The act: workgroup (env blockIdx.x, member blockIdx.y), the row's words in LDS as the rows kernel holds them
// (only the input and the forward's words are touched).  Thread 0 then takes the Q row from the head's words.
__global__ void __launch_bounds__(cg::kRowsThreadsMax) drl_convpop_act_kernel(ActArgs args) {
    (void)args;
    const ActArgs& a = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const cl::Plan& P = a.P;
    extern __shared__ float4 cp_lds4[];
    float* row = reinterpret_cast<float*>(cp_lds4);
    const int tid = threadIdx.x, nt = blockDim.x, m = blockIdx.y;
    const int64_t env = (int64_t)m * a.E + blockIdx.x;  // the env in the batch
    const uint8_t* blk = a.base + a.stride * m;
    const float* online = reinterpret_cast<const float*>(blk + P.pub.online_off);
    const CodeRows cr = {a.row_words, P.code_w};
    for (int i = tid; i < P.in; i += nt) row[i] = dq_input(cr, a.code, env, i);
    __syncthreads();
    const int L = P.n_layers;
    for (int l = 0; l < L; ++l) {
        cl::cl_forward(P, l, online, row);
        __syncthreads();
    }
    const int NA = P.n_actions;
    if (tid == 0) {
        const float* Q = row + P.l[L - 1].delta;
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = i < NA ? Q[i] : 0.0f;
        Epilogue ep;
        ep.seed = a.seed;
        ep.step = a.step;
        ep.env_offset = a.env_offset;
        ep.eps_ptr = a.greedy ? nullptr : &reinterpret_cast<const DqnCounters*>(blk + P.pub.counters_off)->epsilon;
        ep.epsilon = 0.0f;  // (the greedy flag: nothing explores, whatever the member's epsilon)
        ep.actions = a.actions;
        ep.action_stride = a.n_drones;
        ep.q = a.q;
        act_epilogue(ep, env, q, NA, true);
    }
    // drones 1..N-1: drl_synth_actions' columns of this env
    for (int d = 1 + tid; d < a.n_drones; d += nt)
        a.actions[env * a.n_drones + d] = synth_action(a.synth_seed, a.synth_step, (uint64_t)(a.env_offset + env), (uint64_t)d);
}

// ---- the learner: the conv large-batch chain with the member in the grid -------------------------------------
// 1. rows: grid (max_batch, members); the head's deltas divide by the member's batch
__global__ void __launch_bounds__(cg::kRowsThreadsMax) drl_convpop_rows_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ float4 cp_lds4[];
    const Member v = member_of(a, blockIdx.y);
    if (a.size < v.batch) return;  // (uniform over the workgroup, as the row's own bound in the body)
    cg::rows_body(a.P, v, UniformRows{}, v.batch, (int)blockIdx.x, reinterpret_cast<float*>(cp_lds4));
}

// 2. dense partials: grid (dense tiles, chunks of max_batch, members)
__global__ void __launch_bounds__(cg::kThreads) drl_convpop_dense_grad_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) float Xs[cg::kChunkRows * cg::kTileCols];
    __shared__ __attribute__((aligned(16))) float Ds[cg::kChunkRows * cg::kTileUnits];
    const Member v = member_of(a, blockIdx.z);
    const int c = blockIdx.y;
    if (a.size < v.batch || c >= chunks_of(v.batch) || (int)blockIdx.x >= a.t.dense_tiles) return;
    cg::dense_grad_body(a.P, a.t, v, v.batch, (int)blockIdx.x, c, Xs, Ds);
}

// 3. conv partials: grid (parameter groups / kConvWaves, chunks of max_batch, members), a wave per group
__global__ void __launch_bounds__(cg::kThreads) drl_convpop_conv_grad_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Member v = member_of(a, blockIdx.z);
    const int c = blockIdx.y;
    const int gi = __builtin_amdgcn_readfirstlane((int)blockIdx.x * cg::kConvWaves + (int)(threadIdx.x >> 6));
    if (a.size < v.batch || c >= chunks_of(v.batch) || gi >= a.t.conv_groups) return;  // (the whole wave)
    cg::conv_grad_body(a.P, a.t, v, v.batch, gi, c);
}

// 4. update: grid (parameters / kThreads, members), a thread per parameter per member
__global__ void __launch_bounds__(cg::kThreads) drl_convpop_update_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const Member v = member_of(a, blockIdx.y);
    cg::update_body(a.P, a.t, v, a.size >= v.batch ? 1 : 0, chunks_of(v.batch),
                    (int64_t)blockIdx.x * cg::kThreads + threadIdx.x);
}

// 5. counters: a wave per member
__global__ void __launch_bounds__(64) drl_convpop_counters_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ float cs[cg::kMaxChunks];
    const Member v = member_of(a, blockIdx.x);
    cg::counters_body(a.P, v, v.batch, a.size >= v.batch ? 1 : 0, chunks_of(v.batch), nullptr, cs);
}

// The replay slots each member's next train step samples: slots[m][b] for b < the member's batch, -1 beyond.
__global__ void __launch_bounds__(kThreads) drl_convpop_sample_kernel(PopArgs args) {
    (void)args;
    const PopArgs& a = *(const PopArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int m = blockIdx.y, b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= a.P.batch) return;
    const HRec& h = hrec(a.base, a.hp_off, m);
    const DqnCounters* c = reinterpret_cast<const DqnCounters*>(a.base + a.stride * m + a.P.pub.counters_off);
    a.slots[(int64_t)m * a.P.batch + b] = b < h.batch ? dq_sample(h.seed, c->step, b, a.size) : -1;
}

int launch_convpop_init(const PopArgs& a, hipStream_t s) {
    const unsigned gx = (unsigned)((a.P.n_params + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(drl_convpop_init_kernel, dim3(gx, (unsigned)a.members), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

int launch_convpop_act(const ActArgs& a, int threads, hipStream_t s) {
    hipLaunchKernelGGL(drl_convpop_act_kernel, dim3((unsigned)a.E, (unsigned)a.members), dim3((unsigned)threads),
                       (size_t)a.P.row_words * 4, s, a);
    return (int)hipGetLastError();
}

int launch_convpop_train(const PopArgs& a, hipStream_t s) {
    const cl::Plan& P = a.P;
    const unsigned M = (unsigned)a.members, chunks = (unsigned)a.t.chunks;
    hipLaunchKernelGGL(drl_convpop_rows_kernel, dim3((unsigned)P.batch, M), dim3((unsigned)a.t.rows_threads),
                       (size_t)P.row_words * 4, s, a);
    hipLaunchKernelGGL(drl_convpop_dense_grad_kernel, dim3((unsigned)a.t.dense_tiles, chunks, M), dim3(cg::kThreads), 0,
                       s, a);
    hipLaunchKernelGGL(drl_convpop_conv_grad_kernel,
                       dim3((unsigned)((a.t.conv_groups + cg::kConvWaves - 1) / cg::kConvWaves), chunks, M),
                       dim3(cg::kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_convpop_update_kernel, dim3((unsigned)((P.n_params + cg::kThreads - 1) / cg::kThreads), M),
                       dim3(cg::kThreads), 0, s, a);
    hipLaunchKernelGGL(drl_convpop_counters_kernel, dim3(M), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int launch_convpop_sample(const PopArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_convpop_sample_kernel, dim3((unsigned)((a.P.batch + kThreads - 1) / kThreads), (unsigned)a.members),
                       dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace cp
}  // namespace drl
