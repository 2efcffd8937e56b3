// dronerl_per_api.cpp — C ABI of the prioritized replay and its learner (include/dronerl.h drl_per_*,
// drl_dqn_per_train, drl_widenet_dqn_per_train; kernels in dronerl_per.hip, the block's layout in dronerl_per_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_args.h"
#include "../largelearn/dronerl_largelearn_layout.h"
#include "../widenet/dronerl_widenet_layout.h"
#include "dronerl_per_layout.h"
#include "dronerl_per_learn_args.h"

extern "C" __attribute__((visibility("hidden"))) int drl_internal_fail(const char* msg);

namespace {

int fail(const char* m) { return drl_internal_fail(m); }

int hip_fail(int e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString((hipError_t)e));
    return fail(buf);
}

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

// What drl_dqn_per_train and drl_widenet_dqn_per_train share behind their plans (a.P): every check of the
// hyperparameters, the blocks and the ring, then the chain's arguments, the tree's view and the sampler's.
int per_learn_args(drl::per::LearnArgs& a, int in_features, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                   void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                   drl::per::TreeArgs* t, drl::per::SampleArgs* sa) {
    const char* msg = drl::per::learn_args(a, in_features, h, ph, d_agent, d_packed, r, size, d_per, t, sa);
    return msg ? fail(msg) : 0;
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
    drl::QnetLayout L;
    drl::per::LearnArgs a{};
    if (drl::qnet_layout_of(d, &L)) return -1;
    if (!h) return fail("hparams is NULL");
    if (const char* msg = drl::ll::plan(L.n_layers, L.in, L.out, L.code_w, h->batch, &a.P)) return fail(msg);
    const drl::ll::Plan& P = a.P;
    drl::per::TreeArgs t;
    drl::per::SampleArgs sa;
    if (per_learn_args(a, d->in_features, h, ph, d_agent, d_packed, r, size, d_per, &t, &sa)) return -1;
    // the act's image of the new online set, as drl_dqn_large_train refreshes it
    const float* w[drl::QN_MAX_LAYERS] = {};
    const float* b[drl::QN_MAX_LAYERS] = {};
    for (int l = 0; l < P.n_layers; ++l) {
        w[l] = a.online + P.woff[l];
        b[l] = a.online + P.boff[l];
    }
    drl::QnetPack pk;
    drl::qnet_pack_args(L, d_packed, w, b, &pk);
    a.pack_status = reinterpret_cast<uint32_t*>(pk.status);
    if (const int e = drl::per::launch_per_train(a, t, sa, stream); e != 0)
        return hip_fail(e, "drl_dqn_per_train launch");
    const hipError_t e = drl::launch_qnet_pack(pk, stream);
    return e == hipSuccess ? 0 : hip_fail((int)e, "drl_dqn_per_train pack launch");
}

// drl_dqn_per_train on a plan with the wide family's width limit (what drl_widenet_dqn_train is to
// drl_dqn_large_train), then the wide pack kernel.
int drl_widenet_dqn_per_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                              hipStream_t stream) {
    drl::wn::PackArgs pk;
    memset(&pk, 0, sizeof pk);
    drl::per::LearnArgs a{};
    if (const char* msg = drl::wn::layout(d, &pk.L)) return fail(msg);
    if (!h) return fail("hparams is NULL");
    int32_t in[drl::wn::kMaxLayers], out[drl::wn::kMaxLayers];
    for (int l = 0; l < pk.L.n_layers; ++l) {
        in[l] = pk.L.l[l].in;
        out[l] = pk.L.l[l].out;
    }
    if (const char* msg = drl::ll::plan(pk.L.n_layers, in, out, pk.L.code_w, h->batch, &a.P, drl::wn::kMaxWidth))
        return fail(msg);
    const drl::ll::Plan& P = a.P;
    drl::per::TreeArgs t;
    drl::per::SampleArgs sa;
    if (per_learn_args(a, d->in_features, h, ph, d_agent, d_packed, r, size, d_per, &t, &sa)) return -1;
    // the act's image of the new online set, as drl_widenet_dqn_train refreshes it
    for (int l = 0; l < P.n_layers; ++l) {
        pk.w[l] = a.online + P.woff[l];
        pk.b[l] = a.online + P.boff[l];
    }
    pk.packed = static_cast<uint32_t*>(d_packed);
    a.pack_status = pk.packed + pk.L.status;
    if (const int e = drl::per::launch_per_train(a, t, sa, stream); e != 0)
        return hip_fail(e, "drl_widenet_dqn_per_train launch");
    const int e = drl::wn::launch_widenet_pack(pk, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_widenet_dqn_per_train pack launch");
}

}  // extern "C"
