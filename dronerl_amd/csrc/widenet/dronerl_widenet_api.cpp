// dronerl_widenet_api.cpp — C ABI of the wide dense Q-networks (include/dronerl.h drl_widenet_*; kernels in
// dronerl_widenet.hip, layout in dronerl_widenet_layout.h).  The learner calls are the shared front end's
// (../dronerl_learn_front.h) on the wide family: the large-batch learner's launch chain (largelearn/) on a plan
// with this family's width limit, then the wide pack kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_front.h"
#include "dronerl_widenet_layout.h"

namespace front = drl::front;
using drl::fail;
using drl::hip_fail;

namespace {

// Every limit is checked here, by every call: nothing is refused at launch.
int wn_layout(const drl_widenet_desc* d, drl::wn::Layout* L) {
    const char* msg = drl::wn::layout(d, L);
    return msg ? fail(msg) : 0;
}

int num_cus() {
    static std::mutex mu;
    static std::vector<int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> g(mu);
    if ((int)cache.size() <= dev) cache.resize(dev + 1, 0);
    if (!cache[dev]) {
        int n = 0;
        cache[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }
    return cache[dev];
}

}  // namespace

extern "C" {

int drl_widenet_packed_bytes(const drl_widenet_desc* d, int64_t* bytes) {
    drl::wn::Layout L;
    if (wn_layout(d, &L)) return -1;
    if (!bytes) return fail("bytes is NULL");
    *bytes = (int64_t)L.total_words * 4;
    return 0;
}

int drl_widenet_pack(const drl_widenet_desc* d, const float* const* d_weights, const float* const* d_biases,
                     void* d_packed, hipStream_t stream) {
    drl::wn::PackArgs a;
    memset(&a, 0, sizeof a);
    if (wn_layout(d, &a.L)) return -1;
    if (!d_weights || !d_biases || !d_packed) return fail("weights/biases/packed must be non-NULL");
    if ((uintptr_t)d_packed % 16) return fail("packed buffer must be 16-byte aligned");
    for (int l = 0; l < a.L.n_layers; ++l) {
        if (!d_weights[l] || !d_biases[l]) return fail("a weight or bias pointer is NULL");
        a.w[l] = d_weights[l];
        a.b[l] = d_biases[l];
    }
    a.packed = static_cast<uint32_t*>(d_packed);
    if (hipError_t e0 = hipMemsetAsync(a.packed + a.L.status, 0, 16, stream); e0 != hipSuccess)
        return hip_fail((int)e0, "drl_widenet_pack status reset");
    const int e = drl::wn::launch_widenet_pack(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_widenet_pack launch");
}

int drl_widenet_act(const drl_widenet_desc* d, const void* d_packed, const void* d_input, int64_t num_envs,
                    int64_t obs_stride, float epsilon, const float* d_epsilon, uint64_t seed, uint64_t step,
                    int64_t env_offset, int32_t* d_actions, int64_t action_stride, float* d_q, int32_t* d_err,
                    hipStream_t stream) {
    drl::wn::ActArgs a;
    memset(&a, 0, sizeof a);
    if (wn_layout(d, &a.L)) return -1;
    if (num_envs < 0) return fail("num_envs < 0");
    if (num_envs == 0) return 0;
    if (!d_packed || !d_input || !d_actions) return fail("packed/input/actions must be non-NULL");
    if ((uintptr_t)d_packed % 16) return fail("packed buffer must be 16-byte aligned");
    if (a.L.input == DRL_QNET_INPUT_CODE) {
        if ((uintptr_t)d_input % 16) return fail("the policy code must be 16-byte aligned");
    } else {
        if ((uintptr_t)d_input % 8 || obs_stride % 2) return fail("obs rows must be 8-byte aligned (even obs_stride)");
        if (obs_stride < d->in_features) return fail("obs_stride < in_features");
    }
    if ((uintptr_t)d_epsilon % 4) return fail("d_epsilon must be 4-byte aligned");
    if ((uintptr_t)d_actions % 4 || (uintptr_t)d_q % 4 || (uintptr_t)d_err % 4)
        return fail("actions, q and err must be 4-byte aligned");
    if (action_stride < 1) return fail("action_stride must be >= 1");
    a.packed = static_cast<const uint32_t*>(d_packed);
    a.input = d_input;
    a.obs_stride = obs_stride;
    a.E = num_envs;
    a.epsilon = epsilon;
    a.eps_ptr = d_epsilon;
    a.seed = seed;
    a.step = step;
    a.env_offset = env_offset;
    a.actions = d_actions;
    a.action_stride = action_stride;
    a.q = d_q;
    a.err = d_err;
    a.n_actions = a.L.n_actions;
    const int e = drl::wn::launch_widenet_act(a, num_cus(), stream);
    return e == 0 ? 0 : hip_fail(e, "drl_widenet_act launch");
}

int drl_widenet_dqn_layout_query(const drl_widenet_desc* d, int32_t batch, drl_dqn_layout* layout) {
    return front::layout_query<front::Wide>(d, batch, layout);
}

int drl_widenet_dqn_init(const drl_widenet_desc* d, int32_t batch, void* d_agent, float epsilon_start,
                         hipStream_t stream) {
    return front::init<front::Wide>("drl_widenet_dqn_init", d, batch, d_agent, epsilon_start, stream);
}

int drl_widenet_dqn_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                          const drl_replay* r, int64_t size, hipStream_t stream) {
    return front::train<front::Wide, drl::ll::LearnArgs, front::NullHparams::kPlanAtBatch1>(
        "drl_widenet_dqn_train", d, h, nullptr, d_agent, d_packed, r, size, nullptr, stream,
        front::uniform<drl::ll::LearnArgs, drl::ll::launch_large_train>);
}

int drl_widenet_dqn_sample_rows(const drl_widenet_desc* d, const drl_dqn_hparams* h, const void* d_agent,
                                int64_t size, int64_t* d_slots, hipStream_t stream) {
    return front::sample_rows<front::Wide>("drl_widenet_dqn_sample_rows", d, h, d_agent, size, d_slots, stream);
}

}  // extern "C"
