// dronerl_population_member.h — a dense population member's view (device only): the fields the large-batch
// chain's bodies and dronerl_learn_common.h read (ll::LearnArgs' names), built in a kernel from the population's
// arguments and the member's hyperparameter record.  Shared by the population's kernels (dronerl_population.hip)
// and the prioritized population's (perpop/dronerl_perpop.hip), so a member is the same view under both; the
// record's copy (hparams_into) also by the conv population's (convpop/dronerl_convpop.hip), whose records are
// pop::HRec too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "dronerl_population_layout.h"

namespace drl {
namespace pop {

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

// The record's hyperparameters into a member's view (any struct with ll::LearnArgs' names for them)
template <class V>
__device__ __forceinline__ void hparams_into(const HRec& h, V& v) {
    v.gamma = h.gamma;
    v.b1 = h.b1;
    v.b2 = h.b2;
    v.c1 = h.c1;
    v.c2 = h.c2;
    v.adam_eps = h.adam_eps;
    v.neg_lr = h.neg_lr;
    v.tau = h.tau;
    v.one_minus_tau = h.one_minus_tau;
    v.eps_decay = h.eps_decay;
    v.eps_end = h.eps_end;
    v.b1d = h.b1d;
    v.b2d = h.b2d;
    v.target_every = h.target_every;
    v.eps_every = h.eps_every;
}

__device__ __forceinline__ Member member_of(const PopArgs& a, int m) {
    const ll::Plan& P = a.P;
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
    hparams_into(h, v);
    return v;
}

}  // namespace pop
}  // namespace drl
