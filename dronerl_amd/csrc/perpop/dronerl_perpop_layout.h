// dronerl_perpop_layout.h — the prioritized replay of a population of dense DQN agents (include/dronerl.h
// drl_pop_per_*): `members` prioritized blocks at a fixed stride, each laid out exactly as drl_per_layout_query
// lays out one agent for (capacity, max_batch) -- tree[2P], pmax, wmax, slots, weights, |d|; member m uses the
// first batch_m entries of the three arrays -- then one record of PER hyperparameters per member.  The rings, the
// cursor and the size are the population's (population/dronerl_population_layout.h).  Plain C++ (no HIP): the
// host API, the kernels and tests/native/perpop_layout_check.cpp share it.
#ifndef DRONERL_PERPOP_LAYOUT_H
#define DRONERL_PERPOP_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../per/dronerl_per_layout.h"
#include "../population/dronerl_population_layout.h"

namespace drl {
namespace perpop {

constexpr int kMaxMembers = pop::kMaxMembers;
constexpr int kThreads = per::kThreads;

// A member's PER hyperparameters on the device (a drl_per_hparams' values)
struct PRec {
    double alpha, beta0, eps;
    int64_t beta_steps;
};
static_assert(sizeof(PRec) == 32, "a PER record is 32 bytes");
constexpr int64_t kPRecStride = 32;  // (records 16-byte aligned)

struct Plan {
    per::Plan T;       // a member block's plan at max_batch
    int32_t members, max_batch;
    int64_t stride;    // bytes from one member block to the next (T.pub.bytes: a multiple of 16)
    int64_t hp_off;    // bytes: the PER records, kPRecStride each
    int64_t bytes;
};

// Lay the block out.  Returns nullptr, or the message for drl_last_error.
inline const char* plan(int32_t members, int64_t capacity, int32_t max_batch, Plan* out) {
    if (!out) return "internal: the prioritized population's plan is NULL";
    if (members < 1 || members > kMaxMembers) return "members must be in [1, 1024] (DRL_POP_MAX_MEMBERS)";
    if (max_batch < 1 || max_batch > per::kMaxBatch) return "max_batch must be in [1, 4096] (DRL_DQN_LARGE_MAX_BATCH)";
    *out = Plan{};
    if (const char* msg = per::plan(capacity, max_batch, &out->T)) return msg;
    out->members = members;
    out->max_batch = max_batch;
    out->stride = per::r16(out->T.pub.bytes);
    out->hp_off = out->stride * members;
    out->bytes = out->hp_off + kPRecStride * members;
    return nullptr;
}

// a member's block, and its record
inline int64_t member_off(const Plan& p, int m) { return p.stride * m; }
inline int64_t prec_off(const Plan& p, int m) { return p.hp_off + kPRecStride * m; }

// ---- kernel arguments (dronerl_perpop.hip; launched by dronerl_perpop_api.cpp) ------------------------------
// the trees: what init, mark, rebuild and the sampler read.  gate != 0: a member whose batch (its HRec in the
// population block `pop`) exceeds `size` is skipped, as the train step skips it.
struct TreeSetArgs {
    per::Plan T;
    int32_t members, gate;
    int64_t stride, hp_off;
    uint8_t* base;
    // the population block: the members' hyperparameter records and counters (the sampler and the gate)
    const uint8_t* pop;
    int64_t pop_stride, pop_hp_off, pop_counters_off;
    int64_t size;
};

// the learner's chain: the population's arguments and the trees
struct ChainArgs {
    pop::PopArgs p;
    TreeSetArgs t;
};

// (hipError_t values) stream-ordered launches
int launch_init(const TreeSetArgs& t, hipStream_t s);
int launch_mark(const TreeSetArgs& t, int64_t cursor, int64_t count, hipStream_t s);
int launch_rebuild(const TreeSetArgs& t, hipStream_t s);
int launch_sample(const TreeSetArgs& t, hipStream_t s);
// one learner step of every member: rebuild, sample, rows, forward, TD, priority, backward, update, counters
int launch_train(const ChainArgs& a, hipStream_t s);

}  // namespace perpop
}  // namespace drl
#endif
