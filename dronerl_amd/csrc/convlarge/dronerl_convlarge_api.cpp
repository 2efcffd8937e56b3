// dronerl_convlarge_api.cpp — C ABI of the conv Q-network's learner at replay batches up to 4096
// (include/dronerl.h drl_convnet_dqn_large_*; kernels in dronerl_convlarge.hip, the agent block's layout in
// dronerl_convlarge_layout.h).  The checks and the argument block are drl_convnet_dqn_*'s
// (convlearn/dronerl_convlearn_api.cpp) with this family's batch limit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_args.h"
#include "dronerl_convlarge_layout.h"

extern "C" __attribute__((visibility("hidden"))) int drl_internal_fail(const char* msg);

namespace {

int fail(const char* m) { return drl_internal_fail(m); }

int hip_fail(int e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString((hipError_t)e));
    return fail(buf);
}

// Every limit is checked here, by every call: nothing is refused at launch.
int cg_plan(const drl_convnet_desc* d, int32_t batch, drl::cg::Plan* P) {
    const char* msg = drl::cg::plan(d, batch, P);
    return msg ? fail(msg) : 0;
}

}  // namespace

extern "C" {

int drl_convnet_dqn_large_layout_query(const drl_convnet_desc* d, int32_t batch, drl_convnet_dqn_layout* layout) {
    drl::cg::Plan P;
    if (cg_plan(d, batch, &P)) return -1;
    if (!layout) return fail("layout is NULL");
    *layout = P.c.pub;
    return 0;
}

int drl_convnet_dqn_large_init(const drl_convnet_desc* d, int32_t batch, void* d_agent, float epsilon_start,
                               hipStream_t stream) {
    drl::cg::Plan P;
    if (cg_plan(d, batch, &P)) return -1;
    if (!d_agent || (uintptr_t)d_agent % 16) return fail("the agent block must be a 16-byte aligned device pointer");
    uint8_t* base = static_cast<uint8_t*>(d_agent);
    const drl_convnet_dqn_layout& u = P.c.pub;
    // the moments and the counters (the init kernel then sets the counters); the scratch needs no clearing:
    // a step writes every word of it that it reads
    if (hipError_t e = hipMemsetAsync(base + u.m_off, 0, (size_t)(u.scratch_off - u.m_off), stream); e != hipSuccess)
        return hip_fail((int)e, "drl_convnet_dqn_large_init moments and counters");
    hipError_t e = drl::launch_dqn_init(base + u.counters_off, epsilon_start, stream);
    return e == hipSuccess ? 0 : hip_fail((int)e, "drl_convnet_dqn_large_init launch");
}

int drl_convnet_dqn_large_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                                const drl_replay* r, int64_t size, hipStream_t stream) {
    drl::cg::Plan plan;
    if (!h) {
        if (cg_plan(d, 1, &plan)) return -1;
        return fail("hparams is NULL");
    }
    if (cg_plan(d, h->batch, &plan)) return -1;
    drl::cg::LearnArgs full;
    memset(&full, 0, sizeof full);
    full.t = plan.t;
    drl::cl::LearnArgs& a = full.a;
    a.P = plan.c;
    const drl::cl::Plan& P = a.P;
    if (const char* msg = drl::check_learn_call(h, d_agent, d_packed, r)) return fail(msg);
    if (r->capacity < 1 || r->capacity >= ((int64_t)1 << 31)) return fail("replay capacity must be in [1, 2^31)");
    if (size < 0 || size > r->capacity) return fail("size must be in [0, capacity]");
    if (const char* msg = drl::check_learn_rows(r, P.code_w, P.in, "replay obs_floats < window * window * 6"))
        return fail(msg);
    drl::fill_learn_args(a, P.pub, P.code_w, h, d_agent, r, size);
    // the act's image of the new online set: the pack kernel itself on the online set, so the image is a fresh
    // drl_convnet_pack's byte for byte; the counters kernel has stored the status vector's zeros, so a captured
    // call holds kernel nodes only (DESIGN.md §4 "Conv learner")
    drl::cv::PackArgs pk;
    memset(&pk, 0, sizeof pk);
    if (const char* msg = drl::cv::layout(d, &pk.L)) return fail(msg);
    for (int l = 0; l < P.n_layers; ++l) {
        pk.w[l] = a.online + P.l[l].woff;
        pk.b[l] = a.online + P.l[l].boff;
    }
    pk.packed = static_cast<uint32_t*>(d_packed);
    a.pack_status = pk.packed + pk.L.status;
    if (const int e = drl::cg::launch_convlarge_train(full, stream); e != 0)
        return hip_fail(e, "drl_convnet_dqn_large_train launch");
    const int e = drl::cv::launch_convnet_pack(pk, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convnet_dqn_large_train pack launch");
}

int drl_convnet_dqn_large_sample_rows(const drl_convnet_desc* d, const drl_dqn_hparams* h, const void* d_agent,
                                      int64_t size, int64_t* d_slots, hipStream_t stream) {
    drl::cg::Plan P;
    if (!h) {
        if (cg_plan(d, 1, &P)) return -1;
        return fail("hparams is NULL");
    }
    if (cg_plan(d, h->batch, &P)) return -1;
    if (!d_agent || (uintptr_t)d_agent % 16) return fail("the agent block must be a 16-byte aligned device pointer");
    if (!d_slots || (uintptr_t)d_slots % 8) return fail("d_slots must be an 8-byte aligned device pointer");
    if (size < 1) return fail("size must be >= 1 (buffers.py can_sample: nothing is drawn from an empty ring)");
    const int e = drl::cg::launch_convlarge_sample(static_cast<const uint8_t*>(d_agent) + P.c.pub.counters_off,
                                                   h->sample_seed, h->batch, size, d_slots, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convnet_dqn_large_sample_rows launch");
}

}  // extern "C"
