// dronerl_convper_api.cpp — C ABI of the prioritized conv learner (include/dronerl.h drl_convnet_dqn_per_train;
// kernels in dronerl_convper.hip).  The agent block and its checks are drl_convnet_dqn_large_train's
// (convlarge/), the prioritized block and its checks drl_dqn_per_train's (per/).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_args.h"
#include "dronerl_convper_layout.h"

extern "C" __attribute__((visibility("hidden"))) int drl_internal_fail(const char* msg);

namespace {

int fail(const char* m) { return drl_internal_fail(m); }

int hip_fail(int e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString((hipError_t)e));
    return fail(buf);
}

}  // namespace

extern "C" {

// Every limit is checked here, before any device work: nothing is refused at launch.
int drl_convnet_dqn_per_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                              hipStream_t stream) {
    drl::cg::Plan plan;
    if (const char* msg = drl::cg::plan(d, h ? h->batch : 1, &plan)) return fail(msg);
    if (!h) return fail("hparams is NULL");
    drl::cper::LearnArgs full;
    memset(&full, 0, sizeof full);
    full.c.t = plan.t;
    drl::cl::LearnArgs& a = full.c.a;
    a.P = plan.c;
    const drl::cl::Plan& P = a.P;
    if (const char* msg = drl::per::check_hparams(ph)) return fail(msg);
    if (const char* msg = drl::check_learn_call(h, d_agent, d_packed, r)) return fail(msg);
    drl::per::Plan T;
    if (const char* msg = drl::per::plan(r->capacity, h->batch, &T)) return fail(msg);
    if (!d_per || (uintptr_t)d_per % 16)
        return fail("the prioritized replay block must be a 16-byte aligned device pointer");
    if (size < 0 || size > r->capacity) return fail("size must be in [0, capacity]");
    if (const char* msg = drl::check_learn_rows(r, P.code_w, P.in, "replay obs_floats < window * window * 6"))
        return fail(msg);
    drl::fill_learn_args(a, P.pub, P.code_w, h, d_agent, r, size);
    const drl::per::TreeArgs t = drl::per::tree_args(T, d_per);
    full.d = drl::per::drawn_of(t, ph->alpha, ph->eps);
    const drl::per::SampleArgs sa = {h->sample_seed, size, ph->beta0, ph->beta_steps};
    // the act's image of the new online set, as drl_convnet_dqn_large_train refreshes it: the pack kernel on the
    // online set behind the counters kernel's store of the status vector's zeros (kernel nodes only)
    drl::cv::PackArgs pk;
    memset(&pk, 0, sizeof pk);
    if (const char* msg = drl::cv::layout(d, &pk.L)) return fail(msg);
    for (int l = 0; l < P.n_layers; ++l) {
        pk.w[l] = a.online + P.l[l].woff;
        pk.b[l] = a.online + P.l[l].boff;
    }
    pk.packed = static_cast<uint32_t*>(d_packed);
    a.pack_status = pk.packed + pk.L.status;
    if (const int e = drl::cper::launch_convper_train(full, t, sa, stream); e != 0)
        return hip_fail(e, "drl_convnet_dqn_per_train launch");
    const int e = drl::cv::launch_convnet_pack(pk, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convnet_dqn_per_train pack launch");
}

}  // extern "C"
