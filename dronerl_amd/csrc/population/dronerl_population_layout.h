// dronerl_population_layout.h — a population of dense DQN agents in one allocation (include/dronerl.h drl_pop_*):
// `members` agent blocks at a fixed stride, each laid out exactly as drl_dqn_large_layout_query lays out one
// agent for `max_batch` (four parameter sets, the counters, the launch chain's scratch: ll::plan with the wide
// family's width limit), then one hyperparameter record per member.  Plain C++ (no HIP): the host API, the
// kernels and tests/native/population_layout_check.cpp share it.
#ifndef DRONERL_POPULATION_LAYOUT_H
#define DRONERL_POPULATION_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../largelearn/dronerl_largelearn_layout.h"

namespace drl {
namespace pop {

constexpr int kMaxMembers = DRL_POP_MAX_MEMBERS;
constexpr int kMaxWidth = DRL_WIDENET_MAX_WIDTH;  // the hidden widths' limit (no kernel of the chain depends on it)
constexpr int kThreads = ll::kThreads;            // the element-wise kernels' workgroup (the chain's bodies count on it)
// the act: a workgroup of kActThreads takes kActEnvs envs of one member, a thread one unit of the layer at hand
// (kActThreads >= kMaxWidth), kActGroup envs' sums in registers at a time
constexpr int kActThreads = 256, kActEnvs = 16, kActGroup = 8;
static_assert(kActThreads >= kMaxWidth && kActEnvs % kActGroup == 0 && kActThreads >= kActEnvs, "the act's tiling");

// A member's hyperparameters on the device, in the forms ll::LearnArgs carries (the python floats as jax's weak
// typing rounds them into f32 arithmetic; beta1 and beta2 also as doubles for the running powers).
struct HRec {
    int32_t batch, target_every, eps_every, reserved;
    float gamma, b1, b2, c1, c2, adam_eps, neg_lr, tau, one_minus_tau, eps_decay, eps_end, eps_start;  // (eps_start: read by the init kernel alone)
    double b1d, b2d;
    uint64_t seed;
};
static_assert(sizeof(HRec) == 88 && sizeof(HRec) % 8 == 0, "a hyperparameter record is 88 bytes");
constexpr int64_t kHRecStride = 96;  // (records 16-byte aligned)

struct Plan {
    ll::Plan P;              // a member block's plan at max_batch
    int32_t members, n_actions;
    int64_t stride;          // bytes from one member block to the next (P.pub.bytes rounded up to 16)
    int64_t hp_off;          // bytes: the hyperparameter records, kHRecStride each
    int64_t bytes;
    int32_t act_ldx, act_ldh;  // the act's LDS row strides (floats): the decoded inputs, a hidden layer
    int32_t act_lds_bytes;
};

inline int64_t r16(int64_t v) { return (v + 15) / 16 * 16; }

// The host-side record of a drl_dqn_hparams (validated by the caller)
inline HRec hrec_of(const drl_dqn_hparams& h) {
    HRec r = {};
    r.batch = h.batch;
    r.target_every = h.target_update_interval;
    r.eps_every = h.epsilon_decay_every;
    r.gamma = (float)h.gamma;
    r.b1 = (float)h.beta1;
    r.b2 = (float)h.beta2;
    r.c1 = (float)(1.0 - h.beta1);
    r.c2 = (float)(1.0 - h.beta2);
    r.adam_eps = (float)h.adam_eps;
    r.neg_lr = (float)(-h.learning_rate);
    r.tau = (float)h.tau;
    r.one_minus_tau = (float)(1.0 - h.tau);
    r.eps_decay = (float)h.epsilon_decay;
    r.eps_end = (float)h.epsilon_end;
    r.b1d = h.beta1;
    r.b2d = h.beta2;
    r.seed = h.sample_seed;
    return r;
}

// Validate the description (a dense net on the policy code) and lay the population out.  Returns nullptr, or the
// message for drl_last_error.
inline const char* plan(const drl_widenet_desc* d, int32_t members, int32_t max_batch, Plan* out) {
    if (!d) return "the net description is NULL";
    if (!out) return "internal: the population plan is NULL";
    if (d->input != DRL_QNET_INPUT_CODE) return "a population's nets read the policy code (input must be DRL_QNET_INPUT_CODE)";
    int W = 0;
    for (int w = 5; w <= 9; w += 2)
        if (d->in_features == w * w * 6) W = w;
    if (!W) return "in_features must be W*W*6 for a code window W of 5, 7 or 9";
    if (d->n_hidden < 1 || d->n_hidden > 3) return "n_hidden must be 1, 2 or 3";
    for (int l = 0; l < d->n_hidden; ++l)
        if (d->hidden[l] < 8 || d->hidden[l] > kMaxWidth || d->hidden[l] % 8)
            return "hidden widths must be multiples of 8 in [8, 256] (DRL_WIDENET_MAX_WIDTH)";
    if (d->n_actions < 1 || d->n_actions > ll::kMaxActions) return "n_actions must be in [1, 8]";
    if (members < 1 || members > kMaxMembers) return "members must be in [1, 1024] (DRL_POP_MAX_MEMBERS)";
    if (max_batch < 1 || max_batch > ll::kMaxBatch) return "max_batch must be in [1, 4096] (DRL_DQN_LARGE_MAX_BATCH)";
    int32_t in[ll::kMaxLayers], o[ll::kMaxLayers];
    const int L = d->n_hidden + 1;
    for (int l = 0; l < L; ++l) {
        in[l] = l == 0 ? d->in_features : d->hidden[l - 1];
        o[l] = l + 1 < L ? d->hidden[l] : d->n_actions;
    }
    *out = Plan{};
    if (const char* msg = ll::plan(L, in, o, W, max_batch, &out->P, kMaxWidth)) return msg;
    out->members = members;
    out->n_actions = d->n_actions;
    out->stride = r16(out->P.pub.bytes);
    out->hp_off = out->stride * members;
    out->bytes = out->hp_off + kHRecStride * members;
    int hmax = 8;
    for (int l = 0; l < L; ++l) hmax = out->P.ld[l] > hmax ? out->P.ld[l] : hmax;
    out->act_ldx = out->P.in4;
    out->act_ldh = hmax;
    out->act_lds_bytes = 4 * kActEnvs * (out->act_ldx + 2 * out->act_ldh);
    return nullptr;
}

// a member's block, and its record
inline int64_t member_off(const Plan& p, int m) { return p.stride * m; }
inline int64_t hrec_off(const Plan& p, int m) { return p.hp_off + kHRecStride * m; }

// ---- kernel arguments (dronerl_population.hip; launched by dronerl_population_api.cpp) ---------------------
struct PopArgs {
    ll::Plan P;
    int32_t members, n_actions;
    int64_t stride, hp_off;
    uint8_t* base;
    // the rings: [members][capacity] rows of row_words words, actions, rewards, dones
    uint32_t* r_obs;
    uint32_t* r_next;
    int32_t* r_act;
    float* r_rew;
    uint8_t* r_done;
    int64_t capacity, row_words, size;
    int64_t* slots;  // the sample kernel's output, [members][P.batch]
};

struct ActArgs {
    ll::Plan P;
    int32_t members, n_actions;
    int64_t stride, hp_off;
    const uint8_t* base;
    const uint32_t* code;  // [members * E][row_words]
    int64_t row_words, E;  // E: envs per member
    int32_t greedy, ldx, ldh;
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;      // [members * E][n_drones]
    int32_t n_drones;
    uint64_t synth_seed, synth_step;
    float* q;              // nullable: [members * E][n_actions]
};

struct AddArgs {
    uint32_t* r_obs;
    uint32_t* r_next;
    int32_t* r_act;
    float* r_rew;
    uint8_t* r_done;
    int64_t capacity, row_words, cursor, E, total;  // E: envs per member; total = members * E
    const uint32_t* code_prev;
    const uint32_t* code;
    const int32_t* actions;
    const float* rewards;
    const uint8_t* dones;
    int32_t n_drones;
};

// (hipError_t values)
int launch_pop_init(const PopArgs& a, hipStream_t s);  // (the records are in place)
int launch_pop_act(const ActArgs& a, int lds_bytes, hipStream_t s);
int launch_pop_add(const AddArgs& a, hipStream_t s);
int launch_pop_train(const PopArgs& a, hipStream_t s);
// ... and the segments of that chain which the prioritized population's chain (perpop/) launches as they are:
// every layer's forward; the backward pass and the update; the counters.  (No error is read: the caller reads
// hipGetLastError behind its last launch.)  The Double DQN population's chain (doubledqn/) takes the rows too.
void launch_pop_rows(const PopArgs& a, hipStream_t s);
void launch_pop_forward(const PopArgs& a, hipStream_t s);
void launch_pop_backward_update(const PopArgs& a, hipStream_t s);
void launch_pop_counters(const PopArgs& a, hipStream_t s);
int launch_pop_sample(const PopArgs& a, hipStream_t s);
// (host, dronerl_population_api.cpp) drl_pop_train's checks behind its plan, then its argument block: 0, or -1 with
// the message for drl_last_error set
__attribute__((visibility("hidden"))) int pop_train_args(PopArgs* a, const Plan& P, void* d_pop, const drl_replay* r,
                                                         int64_t size);

}  // namespace pop
}  // namespace drl
#endif
