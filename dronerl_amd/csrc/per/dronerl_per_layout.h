// dronerl_per_layout.h — the prioritized replay's device block (include/dronerl.h drl_per_*): the priority sum
// tree over a replay ring's slots, the largest priority ever assigned, and the rows one learner step draws (their
// slots, importance weights and |TD error|).  Plain C++ (no HIP): the host API, the kernels and
// tests/native/per_layout_check.cpp share it.
//
// The tree: P = the smallest power of two >= capacity; float tree[2P] in heap order -- tree[1] the root, node i's
// children 2i and 2i + 1, slot s's leaf tree[P + s], tree[0] unused.  A leaf holds the slot's priority already
// raised to alpha (0.0: never written, or a pad leaf s >= capacity); every internal node is tree[2i] + tree[2i+1]
// as one f32 addition, so a node's bits do not depend on who computes it.
#ifndef DRONERL_PER_LAYOUT_H
#define DRONERL_PER_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../largelearn/dronerl_largelearn_layout.h"

#if defined(__HIPCC__)
#define DRL_PER_HD __host__ __device__ inline
#else
#define DRL_PER_HD inline
#endif

namespace drl {
namespace per {

constexpr int64_t kMaxCapacity = DRL_PER_MAX_CAPACITY;  // 2^24 slots
constexpr int kMaxBatch = DRL_DQN_LARGE_MAX_BATCH;
// the rebuild kernel: a workgroup of kRebuildThreads reduces a run of up to kRun consecutive nodes of one level
// through LDS (a heap of 2 * kRun floats) and writes every level of that subtree; the top of a tree of more than
// kRun leaves is one more such subtree over the runs' roots (P / kRun <= kRun of them)
constexpr int kRun = 4096, kRebuildThreads = 256;
static_assert(kMaxCapacity / kRun <= kRun, "two launches rebuild the largest tree");
// the sample kernel: one workgroup, a thread per kSampleRows rows, the tree's nodes below kTop in LDS
constexpr int kSampleThreads = 1024, kSampleRows = kMaxBatch / kSampleThreads, kTop = 4096;
constexpr int kThreads = 256;  // the element-wise kernels' workgroup
static_assert(kThreads == ll::kThreads, "the chain's counters body is written for the element-wise workgroup");
constexpr float kMaxPriority = 18446744073709551616.0f;  // 2^64: a priority's clamp (and a NaN's value)

DRL_PER_HD int64_t r16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// the smallest power of two >= capacity (capacity in [1, 2^24])
DRL_PER_HD int64_t leaves_of(int64_t capacity) {
    int64_t p = 1;
    while (p < capacity) p <<= 1;
    return p;
}

struct Plan {
    int64_t capacity, P;
    int32_t batch, logP;
    drl_per_layout pub;
};

// Lay the block out.  Returns nullptr, or the message for drl_last_error.
inline const char* plan(int64_t capacity, int32_t batch, Plan* p) {
    if (!p) return "internal: the prioritized replay's plan is NULL";
    if (capacity < 1 || capacity > kMaxCapacity) return "capacity must be in [1, 2^24] (DRL_PER_MAX_CAPACITY)";
    if (batch < 1 || batch > kMaxBatch) return "batch must be in [1, 4096] (DRL_DQN_LARGE_MAX_BATCH)";
    *p = Plan{};
    p->capacity = capacity;
    p->P = leaves_of(capacity);
    p->batch = batch;
    for (int64_t v = p->P; v > 1; v >>= 1) ++p->logP;
    drl_per_layout& o = p->pub;
    o.capacity = capacity;
    o.leaves = p->P;
    o.batch = batch;
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t off = at;
        at += r16(bytes);
        return off;
    };
    o.tree_off = take(2 * p->P * 4);
    o.pmax_off = take(4);
    o.wmax_off = take(4);
    o.slots_off = take((int64_t)batch * 8);
    o.weights_off = take((int64_t)batch * 4);
    o.absd_off = take((int64_t)batch * 4);
    o.bytes = at;
    return nullptr;
}

// The PER hyperparameters' ranges.  Returns nullptr, or the message for drl_last_error.
inline const char* check_hparams(const drl_per_hparams* ph) {
    if (!ph) return "the prioritized replay's hparams are NULL";
    if (!(ph->alpha >= 0.0)) return "alpha must be >= 0";
    if (!(ph->beta0 >= 0.0 && ph->beta0 <= 1.0)) return "beta0 must be in [0, 1]";
    if (ph->beta_steps < 0) return "beta_steps must be >= 0";
    if (!(ph->eps >= 0.0)) return "eps must be >= 0";
    return nullptr;
}

// ---- the rebuild's launches ---------------------------------------------------------------------------------
// the first launch: P / run workgroups, each over `run` leaves; a second one (one workgroup over the P / kRun
// runs' roots) iff P > kRun
DRL_PER_HD int64_t rebuild_run(int64_t P) { return P < kRun ? P : kRun; }
DRL_PER_HD int64_t rebuild_groups(int64_t P) { return P / rebuild_run(P); }

// ---- kernel arguments (dronerl_per.hip; launched by dronerl_per_api.cpp) ------------------------------------
struct TreeArgs {
    float* tree;
    float* pmax;
    float* wmax;
    int64_t* slots;
    float* weights;
    float* absd;
    int64_t capacity, P;
    int32_t batch, logP;
};

DRL_PER_HD TreeArgs tree_args(const Plan& p, void* d_per) {
    uint8_t* base = static_cast<uint8_t*>(d_per);
    TreeArgs t;
    t.tree = reinterpret_cast<float*>(base + p.pub.tree_off);
    t.pmax = reinterpret_cast<float*>(base + p.pub.pmax_off);
    t.wmax = reinterpret_cast<float*>(base + p.pub.wmax_off);
    t.slots = reinterpret_cast<int64_t*>(base + p.pub.slots_off);
    t.weights = reinterpret_cast<float*>(base + p.pub.weights_off);
    t.absd = reinterpret_cast<float*>(base + p.pub.absd_off);
    t.capacity = p.capacity;
    t.P = p.P;
    t.batch = p.batch;
    t.logP = p.logP;
    return t;
}

// what the sampler reads besides the tree
struct SampleArgs {
    uint64_t seed;
    int64_t size;
    double beta0;
    int64_t beta_steps;
};

// One step's drawn rows and the tree's leaves, as the rows, the TD and the priority kernels of every prioritized
// chain see them (dense, population member, conv): the rows' policy of dronerl_learn_common.h.
struct Drawn {
    const int64_t* slots;  // [batch]: the drawn slots
    const float* weights;  // [batch]: their importance weights, w / wmax
    float* absd;           // [batch]: |q - td| of the rows
    float* leaves;         // tree + P: slot s's leaf is leaves[s]
    float* pmax;
    double alpha, per_eps;
};

DRL_PER_HD Drawn drawn_of(const TreeArgs& t, double alpha, double per_eps) {
    return Drawn{t.slots, t.weights, t.absd, t.tree + t.P, t.pmax, alpha, per_eps};
}

// the learner's: the large-batch chain's arguments (the base: what the uniform kernels of the chain are launched
// with) and the step's drawn rows
struct LearnArgs : ll::LearnArgs {
    Drawn d;
};
static_assert(sizeof(LearnArgs) <= 4096, "the arguments are read in place from the kernarg segment");

// (hipError_t values) stream-ordered launches
int launch_init(const TreeArgs& t, hipStream_t s);
int launch_mark(const TreeArgs& t, int64_t cursor, int64_t count, hipStream_t s);
int launch_rebuild(const TreeArgs& t, hipStream_t s);
int launch_sample(const TreeArgs& t, const SampleArgs& a, const void* counters, hipStream_t s);
// one learner step without the pack: rebuild, sample, the chain with the priority update (a.trained), or the
// chain's no-sample step
int launch_per_train(const LearnArgs& a, const TreeArgs& t, const SampleArgs& sa, hipStream_t s);
// ... and the segments of that chain which the Double DQN chain (doubledqn/) launches as they are: the rows at the
// drawn slots; the priorities.  (No error is read: the caller reads hipGetLastError behind its last launch.)
void launch_per_rows(const LearnArgs& a, hipStream_t s);
void launch_per_priority(const LearnArgs& a, hipStream_t s);

}  // namespace per
}  // namespace drl
#endif
