// dronerl_convnet_api.cpp — C ABI of the conv Q-network's inference half (include/dronerl.h drl_convnet_*;
// kernels in dronerl_convnet.hip, shape arithmetic in dronerl_convnet_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "dronerl_convnet_layout.h"

using drl::fail;
using drl::hip_fail;

namespace {

// Every limit is checked here, by every call: nothing is refused at launch.
int cv_layout(const drl_convnet_desc* d, drl::cv::Layout* L) {
    const char* msg = drl::cv::layout(d, L);
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

int drl_convnet_packed_bytes(const drl_convnet_desc* d, int64_t* bytes) {
    drl::cv::Layout L;
    if (cv_layout(d, &L)) return -1;
    if (!bytes) return fail("bytes is NULL");
    *bytes = (int64_t)L.total_words * 4;
    return 0;
}

int drl_convnet_pack(const drl_convnet_desc* d, const float* const* d_conv_w, const float* const* d_conv_b,
                     const float* const* d_dense_w, const float* const* d_dense_b, void* d_packed, hipStream_t stream) {
    drl::cv::PackArgs a;
    memset(&a, 0, sizeof a);
    if (cv_layout(d, &a.L)) return -1;
    if (!d_conv_w || !d_conv_b || !d_dense_w || !d_dense_b || !d_packed)
        return fail("conv_w/conv_b/dense_w/dense_b/packed must be non-NULL");
    if ((uintptr_t)d_packed % 16) return fail("packed buffer must be 16-byte aligned");
    for (int l = 0; l < a.L.n_layers; ++l) {
        const int j = l - a.L.n_conv;
        a.w[l] = j < 0 ? d_conv_w[l] : d_dense_w[j];
        a.b[l] = j < 0 ? d_conv_b[l] : d_dense_b[j];
        if (!a.w[l] || !a.b[l]) return fail("a weight or bias pointer is NULL");
    }
    a.packed = static_cast<uint32_t*>(d_packed);
    if (hipError_t e0 = hipMemsetAsync(a.packed + a.L.status, 0, 16, stream); e0 != hipSuccess)
        return hip_fail((int)e0, "drl_convnet_pack status reset");
    const int e = drl::cv::launch_convnet_pack(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convnet_pack launch");
}

int drl_convnet_act(const drl_convnet_desc* d, const void* d_packed, const void* d_input, int64_t num_envs,
                    int64_t obs_stride, float epsilon, const float* d_epsilon, uint64_t seed, uint64_t step,
                    int64_t env_offset, int32_t* d_actions, int64_t action_stride, float* d_q, int32_t* d_err,
                    hipStream_t stream) {
    drl::cv::ActArgs a;
    memset(&a, 0, sizeof a);
    if (cv_layout(d, &a.L)) return -1;
    if (num_envs < 0) return fail("num_envs < 0");
    if (num_envs == 0) return 0;
    if (!d_packed || !d_input || !d_actions) return fail("packed/input/actions must be non-NULL");
    if ((uintptr_t)d_packed % 16) return fail("packed buffer must be 16-byte aligned");
    if (a.L.input == DRL_QNET_INPUT_CODE) {
        if ((uintptr_t)d_input % 16) return fail("the policy code must be 16-byte aligned");
    } else {
        if ((uintptr_t)d_input % 8 || obs_stride % 2) return fail("obs rows must be 8-byte aligned (even obs_stride)");
        if (obs_stride < (int64_t)a.L.window * a.L.window * 6) return fail("obs_stride < window * window * 6");
    }
    if ((uintptr_t)d_epsilon % 4) return fail("d_epsilon must be 4-byte aligned");
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
    const int e = drl::cv::launch_convnet_act(a, num_cus(), stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convnet_act launch");
}

}  // extern "C"
