// dronerl_learn_args.h — what the learners' train calls share on the host behind their plans (plain C++, no HIP
// call: tests/native/learn_args_check.cpp runs it on host structs): the checks of the hyperparameters, the blocks
// and the ring, each refusal's text once, and the filling of the chain's argument block.  `A` is any chain
// learner's LearnArgs (ll::LearnArgs, cl::LearnArgs and what derives from them: the same field names, a.P the
// caller's plan), `Pub` its public layout (drl_dqn_layout, drl_convnet_dqn_layout: the same offsets' names).
// Every check returns nullptr, or the message for drl_last_error.  The calls' front end over these is
// dronerl_learn_front.h; the prioritized calls' order of them is per/dronerl_per_learn_args.h.
#ifndef DRONERL_LEARN_ARGS_H
#define DRONERL_LEARN_ARGS_H

#include <stdint.h>

#include "../../include/dronerl.h"
#include "dronerl_internal.h"

namespace drl {

// the two families' names for f32 rows shorter than the net's input (check_learn_rows)
constexpr const char* kShortRowsDense = "replay obs_floats < in_features";
constexpr const char* kShortRowsConv = "replay obs_floats < window * window * 6";

// The ranges of the hyperparameters a learner step reads (the batch is the plan's to check).
inline const char* check_hparam_ranges(const drl_dqn_hparams* h) {
    if (h->target_update_interval < 1 || h->epsilon_decay_every < 1)
        return "target_update_interval and epsilon_decay_every must be >= 1";
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0))
        return "beta1 and beta2 must be in [0, 1)";
    return nullptr;
}

inline const char* check_agent_block(const void* d_agent) {
    if (!d_agent || (uintptr_t)d_agent % 16) return "the agent block must be a 16-byte aligned device pointer";
    return nullptr;
}

// Who refuses a ring too large for the learner's int32 slot index: check_ring, or, in a prioritized call, the
// tree's plan behind it (per::plan, whose limit is lower and whose message names it).
enum class RingCapacity { kCheckedHere, kLeftToPerPlan };

// The ring's pointers and its capacity.
inline const char* check_ring(const drl_replay* r, RingCapacity cap = RingCapacity::kCheckedHere) {
    if (!r || !r->obs || !r->next_obs || !r->actions || !r->rewards || !r->dones) return "replay buffers are NULL";
    if (cap == RingCapacity::kLeftToPerPlan) return nullptr;
    if (r->capacity < 1 || r->capacity >= ((int64_t)1 << 31)) return "replay capacity must be in [1, 2^31)";
    return nullptr;
}

// The hyperparameters' ranges, the agent block, the packed image and the ring.
inline const char* check_learn_call(const drl_dqn_hparams* h, const void* d_agent, const void* d_packed,
                                    const drl_replay* r, RingCapacity cap) {
    if (const char* msg = check_hparam_ranges(h)) return msg;
    if (const char* msg = check_agent_block(d_agent)) return msg;
    if (!d_packed || (uintptr_t)d_packed % 16) return "packed buffer must be a 16-byte aligned device pointer";
    return check_ring(r, cap);
}

inline const char* check_learn_size(const drl_replay* r, int64_t size) {
    if (size < 0 || size > r->capacity) return "size must be in [0, capacity]";
    return nullptr;
}

// The ring's rows against the net's input: policy codes of window code_w (0: f32 rows of at least in_floats, else
// `short_rows`), 4-byte aligned.
inline const char* check_learn_rows(const drl_replay* r, int code_w, int in_floats, const char* short_rows) {
    if (code_w) {
        if ((int64_t)r->obs_floats * 4 != lay::code_bytes(code_w))
            return "a DRL_QNET_INPUT_CODE net's replay rows are policy codes (drl_policy_code_bytes / 4 words)";
    } else if (r->obs_floats < in_floats) {
        return short_rows;
    }
    if ((uintptr_t)r->obs % 4 || (uintptr_t)r->next_obs % 4) return "replay rows must be 4-byte aligned";
    return nullptr;
}

// Everything of the argument block but the plan (a.P, which the caller has made) and pack_status.
template <class A, class Pub>
inline void fill_learn_args(A& a, const Pub& pub, int code_w, const drl_dqn_hparams* h, void* d_agent,
                            const drl_replay* r, int64_t size) {
    uint8_t* base = static_cast<uint8_t*>(d_agent);
    a.trained = size >= h->batch;  // buffers.py:92-93 can_sample
    a.code_w = code_w;
    a.online = reinterpret_cast<float*>(base + pub.online_off);
    a.target = reinterpret_cast<float*>(base + pub.target_off);
    a.adam_m = reinterpret_cast<float*>(base + pub.m_off);
    a.adam_v = reinterpret_cast<float*>(base + pub.v_off);
    a.ctr = reinterpret_cast<DqnCounters*>(base + pub.counters_off);
    a.scratch = reinterpret_cast<float*>(base + pub.scratch_off);
    a.r_obs = reinterpret_cast<const uint32_t*>(r->obs);
    a.r_next = reinterpret_cast<const uint32_t*>(r->next_obs);
    a.row_words = r->obs_floats;
    a.r_act = r->actions;
    a.r_rew = r->rewards;
    a.r_done = r->dones;
    a.size = size;
    a.seed = h->sample_seed;
    // the python floats as jax's weak typing rounds them into f32 arithmetic
    a.gamma = (float)h->gamma;
    a.b1 = (float)h->beta1;
    a.b2 = (float)h->beta2;
    a.c1 = (float)(1.0 - h->beta1);
    a.c2 = (float)(1.0 - h->beta2);
    a.adam_eps = (float)h->adam_eps;
    a.neg_lr = (float)(-h->learning_rate);
    a.tau = (float)h->tau;
    a.one_minus_tau = (float)(1.0 - h->tau);
    a.eps_decay = (float)h->epsilon_decay;
    a.eps_end = (float)h->epsilon_end;
    a.b1d = h->beta1;
    a.b2d = h->beta2;
    a.target_every = h->target_update_interval;
    a.eps_every = h->epsilon_decay_every;
}

// A uniform train call behind its plan (a.P): every check in the calls' order, then the argument block.  A
// refused call leaves `a` as it was.
template <class A>
inline const char* learn_args(A& a, int in_floats, const char* short_rows, const drl_dqn_hparams* h, void* d_agent,
                              void* d_packed, const drl_replay* r, int64_t size) {
    if (const char* msg = check_learn_call(h, d_agent, d_packed, r, RingCapacity::kCheckedHere)) return msg;
    if (const char* msg = check_learn_size(r, size)) return msg;
    if (const char* msg = check_learn_rows(r, a.P.code_w, in_floats, short_rows)) return msg;
    fill_learn_args(a, a.P.pub, a.P.code_w, h, d_agent, r, size);
    return nullptr;
}

}  // namespace drl
#endif
