// dronerl_per_api.cpp — C ABI of the prioritized replay and its learner (include/dronerl.h drl_per_*,
// drl_dqn_per_train, drl_widenet_dqn_per_train; kernels in dronerl_per.hip, the block's layout in dronerl_per_layout.h).
// The train calls are the shared front end's (../dronerl_learn_front.h) with the prioritized chain.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_front.h"
#include "dronerl_per_layout.h"

namespace front = drl::front;
using drl::fail;
using drl::hip_fail;

namespace {

// Every limit is checked here, by every call: nothing is refused at launch.
int per_plan(int64_t capacity, int32_t batch, drl::per::Plan* P) {
    const char* msg = drl::per::plan(capacity, batch, P);
    return msg ? fail(msg) : 0;
}

int per_block(int64_t capacity, int32_t batch, void* d_per, drl::per::Plan* P) {
    if (per_plan(capacity, batch, P)) return -1;
    if (!d_per || (uintptr_t)d_per % 16) return fail("the prioritized replay block must be a 16-byte aligned device pointer");
    return 0;
}

int per_hparams(const drl_per_hparams* ph) {
    if (const char* msg = drl::per::check_hparams(ph)) return fail(msg);
    return 0;
}

}  // namespace

extern "C" {

int drl_per_layout_query(int64_t capacity, int32_t batch, drl_per_layout* layout) {
    drl::per::Plan P;
    if (per_plan(capacity, batch, &P)) return -1;
    if (!layout) return fail("layout is NULL");
    *layout = P.pub;
    return 0;
}

int drl_per_init(int64_t capacity, int32_t batch, void* d_per, hipStream_t stream) {
    drl::per::Plan P;
    if (per_block(capacity, batch, d_per, &P)) return -1;
    const int e = drl::per::launch_init(drl::per::tree_args(P, d_per), stream);
    return e == 0 ? 0 : hip_fail(e, "drl_per_init launch");
}

int drl_per_mark_new(int64_t capacity, int32_t batch, void* d_per, int64_t cursor, int64_t count, hipStream_t stream) {
    drl::per::Plan P;
    if (per_block(capacity, batch, d_per, &P)) return -1;
    if (cursor < 0 || cursor >= capacity) return fail("cursor must be in [0, capacity)");
    if (count < 0) return fail("count must be >= 0");
    const int e = drl::per::launch_mark(drl::per::tree_args(P, d_per), cursor, count, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_per_mark_new launch");
}

int drl_per_rebuild(int64_t capacity, int32_t batch, void* d_per, hipStream_t stream) {
    drl::per::Plan P;
    if (per_block(capacity, batch, d_per, &P)) return -1;
    const int e = drl::per::launch_rebuild(drl::per::tree_args(P, d_per), stream);
    return e == 0 ? 0 : hip_fail(e, "drl_per_rebuild launch");
}

int drl_per_sample(int64_t capacity, int32_t batch, void* d_per, const drl_per_hparams* ph, uint64_t seed,
                   const void* d_counters, int64_t size, hipStream_t stream) {
    drl::per::Plan P;
    if (per_block(capacity, batch, d_per, &P)) return -1;
    if (per_hparams(ph)) return -1;
    if (!d_counters || (uintptr_t)d_counters % 8) return fail("d_counters must be an 8-byte aligned device pointer");
    if (size < 1 || size > capacity) return fail("size must be in [1, capacity] (nothing is drawn from an empty ring)");
    const drl::per::SampleArgs sa = {seed, size, ph->beta0, ph->beta_steps};
    const int e = drl::per::launch_sample(drl::per::tree_args(P, d_per), sa, d_counters, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_per_sample launch");
}

int drl_dqn_per_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph, void* d_agent,
                      void* d_packed, const drl_replay* r, int64_t size, void* d_per, hipStream_t stream) {
    return front::train<front::Dense, drl::per::LearnArgs, front::NullHparams::kLayoutOnly>(
        "drl_dqn_per_train", d, h, ph, d_agent, d_packed, r, size, d_per, stream, drl::per::launch_per_train);
}

// drl_dqn_per_train on a plan with the wide family's width limit (what drl_widenet_dqn_train is to
// drl_dqn_large_train), then the wide pack kernel.
int drl_widenet_dqn_per_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                              hipStream_t stream) {
    return front::train<front::Wide, drl::per::LearnArgs, front::NullHparams::kLayoutOnly>(
        "drl_widenet_dqn_per_train", d, h, ph, d_agent, d_packed, r, size, d_per, stream, drl::per::launch_per_train);
}

}  // extern "C"
