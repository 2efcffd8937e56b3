// dronerl_convpop_layout.h — a population of conv DQN agents in one allocation (include/dronerl.h drl_convpop_*):
// `members` agent blocks at a fixed stride, each laid out exactly as drl_convnet_dqn_large_layout_query lays out
// one agent for `max_batch` (four parameter sets, the counters, the launch chain's scratch: cg::plan), then one
// hyperparameter record per member (pop::HRec, the dense population's record and stride).  Plain C++ (no HIP):
// the host API, the kernels and tests/native/convpop_layout_check.cpp share it.
#ifndef DRONERL_CONVPOP_LAYOUT_H
#define DRONERL_CONVPOP_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../convlarge/dronerl_convlarge_layout.h"
#include "../population/dronerl_population_layout.h"

namespace drl {
namespace cp {

using pop::HRec;
using pop::kHRecStride;
constexpr int kMaxMembers = DRL_POP_MAX_MEMBERS;
constexpr int kThreads = cg::kThreads;  // the element-wise kernels' workgroup

struct Plan {
    cg::Plan P;  // a member block's plan at max_batch
    int32_t members, code_w;
    int64_t stride;  // bytes from one member block to the next (P.c.pub.bytes rounded up to 16)
    int64_t hp_off;  // bytes: the hyperparameter records, kHRecStride each
    int64_t bytes;
};

// Validate the description (a conv net on the policy code) and lay the population out.  Returns nullptr, or the
// message for drl_last_error.
inline const char* plan(const drl_convnet_desc* d, int32_t members, int32_t max_batch, Plan* out) {
    if (!d) return "the net description is NULL";
    if (!out) return "internal: the population plan is NULL";
    if (d->input != DRL_QNET_INPUT_CODE)
        return "a population's nets read the policy code (input must be DRL_QNET_INPUT_CODE)";
    if (d->window != 5 && d->window != 7 && d->window != 9) return "the code window must be 5, 7 or 9";
    if (members < 1 || members > kMaxMembers) return "members must be in [1, 1024] (DRL_POP_MAX_MEMBERS)";
    if (max_batch < 1 || max_batch > cg::kMaxBatch)
        return "max_batch must be in [1, 4096] (DRL_CONVNET_DQN_LARGE_MAX_BATCH)";
    *out = Plan{};
    if (const char* msg = cg::plan(d, max_batch, &out->P)) return msg;
    out->members = members;
    out->code_w = out->P.c.code_w;
    out->stride = pop::r16(out->P.c.pub.bytes);
    out->hp_off = out->stride * members;
    out->bytes = out->hp_off + kHRecStride * members;
    return nullptr;
}

// a member's block, and its record
inline int64_t member_off(const Plan& p, int m) { return p.stride * m; }
inline int64_t hrec_off(const Plan& p, int m) { return p.hp_off + kHRecStride * m; }

// ---- kernel arguments (dronerl_convpop.hip; launched by dronerl_convpop_api.cpp) ---------------------------
struct PopArgs {
    cl::Plan P;
    cg::Tiles t;
    int32_t members;
    int64_t stride, hp_off;
    uint8_t* base;
    // the rings: [members][capacity] rows of row_words words, actions, rewards, dones
    const uint32_t* r_obs;
    const uint32_t* r_next;
    const int32_t* r_act;
    const float* r_rew;
    const uint8_t* r_done;
    int64_t capacity, row_words, size;
    int64_t* slots;  // the sample kernel's output, [members][P.batch]
};

struct ActArgs {
    cl::Plan P;
    int32_t members;
    int64_t stride;
    const uint8_t* base;
    const uint32_t* code;  // [members * E][row_words]
    int64_t row_words, E;  // E: envs per member
    int32_t greedy;
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;      // [members * E][n_drones]
    int32_t n_drones;
    uint64_t synth_seed, synth_step;
    float* q;              // nullable: [members * E][n_actions]
};

// (hipError_t values)
int launch_convpop_init(const PopArgs& a, hipStream_t s);  // (the records are in place)
int launch_convpop_act(const ActArgs& a, int threads, hipStream_t s);
int launch_convpop_train(const PopArgs& a, hipStream_t s);
int launch_convpop_sample(const PopArgs& a, hipStream_t s);

}  // namespace cp
}  // namespace drl
#endif
