// dronerl_doubledqn_api.cpp — C ABI of the Double DQN learner calls (include/dronerl.h drl_dqn_double_train,
// drl_widenet_dqn_double_train, drl_dqn_double_per_train, drl_widenet_dqn_double_per_train, drl_pop_double_train;
// kernels in dronerl_doubledqn.hip).  Each call makes the checks of its max-rule call through that call's own
// checking function (ll::large_train_args, per::learn_args, pop::pop_train_args), fills that call's argument
// block and launches that call's chain with the Double forward and TD kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_args.h"
#include "../largelearn/dronerl_largelearn_layout.h"
#include "../per/dronerl_per_layout.h"
#include "../per/dronerl_per_learn_args.h"
#include "../population/dronerl_population_layout.h"
#include "../widenet/dronerl_widenet_layout.h"
#include "dronerl_doubledqn.h"

extern "C" __attribute__((visibility("hidden"))) int drl_internal_fail(const char* msg);

namespace {

int fail(const char* m) { return drl_internal_fail(m); }

int hip_fail(int e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString((hipError_t)e));
    return fail(buf);
}

// the dense family's plan (drl_dqn_large_train's)
int ll_plan(const drl_qnet_desc* d, int32_t batch, drl::QnetLayout* L, drl::ll::Plan* P) {
    if (drl::qnet_layout_of(d, L)) return -1;
    const char* msg = drl::ll::plan(L->n_layers, L->in, L->out, L->code_w, batch, P);
    return msg ? fail(msg) : 0;
}

// ... and the wide family's (drl_widenet_dqn_train's)
int wn_plan(const drl_widenet_desc* d, int32_t batch, drl::wn::Layout* L, drl::ll::Plan* P) {
    if (const char* msg = drl::wn::layout(d, L)) return fail(msg);
    int32_t in[drl::wn::kMaxLayers], out[drl::wn::kMaxLayers];
    for (int l = 0; l < L->n_layers; ++l) {
        in[l] = L->l[l].in;
        out[l] = L->l[l].out;
    }
    const char* msg = drl::ll::plan(L->n_layers, in, out, L->code_w, batch, P, drl::wn::kMaxWidth);
    return msg ? fail(msg) : 0;
}

// the act's image of the new online set: the dense pack kernel's arguments (drl_dqn_large_train's refresh)
template <class A>
void dense_pack(const drl::QnetLayout& L, A& a, void* d_packed, drl::QnetPack* pk) {
    const float* w[drl::QN_MAX_LAYERS] = {};
    const float* b[drl::QN_MAX_LAYERS] = {};
    for (int l = 0; l < a.P.n_layers; ++l) {
        w[l] = a.online + a.P.woff[l];
        b[l] = a.online + a.P.boff[l];
    }
    drl::qnet_pack_args(L, d_packed, w, b, pk);
    a.pack_status = reinterpret_cast<uint32_t*>(pk->status);
}

// ... and the wide pack kernel's (drl_widenet_dqn_train's refresh)
template <class A>
void wide_pack(A& a, void* d_packed, drl::wn::PackArgs* pk) {
    for (int l = 0; l < a.P.n_layers; ++l) {
        pk->w[l] = a.online + a.P.woff[l];
        pk->b[l] = a.online + a.P.boff[l];
    }
    pk->packed = static_cast<uint32_t*>(d_packed);
    a.pack_status = pk->packed + pk->L.status;
}

}  // namespace

extern "C" {

int drl_dqn_double_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                         const drl_replay* r, int64_t size, hipStream_t stream) {
    drl::QnetLayout L;
    drl::ll::LearnArgs a;
    memset(&a, 0, sizeof a);
    if (!h) {
        if (ll_plan(d, 1, &L, &a.P)) return -1;
        return fail("hparams is NULL");
    }
    if (ll_plan(d, h->batch, &L, &a.P)) return -1;
    if (drl::ll::large_train_args(a, d->in_features, h, d_agent, d_packed, r, size)) return -1;
    drl::QnetPack pk;
    dense_pack(L, a, d_packed, &pk);
    if (const int e = drl::dd::launch_double_train(a, stream); e != 0) return hip_fail(e, "drl_dqn_double_train launch");
    const hipError_t e = drl::launch_qnet_pack(pk, stream);
    return e == hipSuccess ? 0 : hip_fail((int)e, "drl_dqn_double_train pack launch");
}

int drl_widenet_dqn_double_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                                 const drl_replay* r, int64_t size, hipStream_t stream) {
    drl::wn::PackArgs pk;
    memset(&pk, 0, sizeof pk);
    drl::ll::LearnArgs a;
    memset(&a, 0, sizeof a);
    if (!h) {
        if (wn_plan(d, 1, &pk.L, &a.P)) return -1;
        return fail("hparams is NULL");
    }
    if (wn_plan(d, h->batch, &pk.L, &a.P)) return -1;
    if (drl::ll::large_train_args(a, d->in_features, h, d_agent, d_packed, r, size)) return -1;
    wide_pack(a, d_packed, &pk);
    if (const int e = drl::dd::launch_double_train(a, stream); e != 0)
        return hip_fail(e, "drl_widenet_dqn_double_train launch");
    const int e = drl::wn::launch_widenet_pack(pk, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_widenet_dqn_double_train pack launch");
}

int drl_dqn_double_per_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                             void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                             hipStream_t stream) {
    drl::QnetLayout L;
    drl::per::LearnArgs a{};
    if (drl::qnet_layout_of(d, &L)) return -1;
    if (!h) return fail("hparams is NULL");
    if (const char* msg = drl::ll::plan(L.n_layers, L.in, L.out, L.code_w, h->batch, &a.P)) return fail(msg);
    drl::per::TreeArgs t;
    drl::per::SampleArgs sa;
    if (const char* msg = drl::per::learn_args(a, d->in_features, h, ph, d_agent, d_packed, r, size, d_per, &t, &sa))
        return fail(msg);
    drl::QnetPack pk;
    dense_pack(L, a, d_packed, &pk);
    if (const int e = drl::dd::launch_double_per_train(a, t, sa, stream); e != 0)
        return hip_fail(e, "drl_dqn_double_per_train launch");
    const hipError_t e = drl::launch_qnet_pack(pk, stream);
    return e == hipSuccess ? 0 : hip_fail((int)e, "drl_dqn_double_per_train pack launch");
}

int drl_widenet_dqn_double_per_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
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
    drl::per::TreeArgs t;
    drl::per::SampleArgs sa;
    if (const char* msg = drl::per::learn_args(a, d->in_features, h, ph, d_agent, d_packed, r, size, d_per, &t, &sa))
        return fail(msg);
    wide_pack(a, d_packed, &pk);
    if (const int e = drl::dd::launch_double_per_train(a, t, sa, stream); e != 0)
        return hip_fail(e, "drl_widenet_dqn_double_per_train launch");
    const int e = drl::wn::launch_widenet_pack(pk, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_widenet_dqn_double_per_train pack launch");
}

int drl_pop_double_train(const drl_widenet_desc* d, int32_t members, int32_t max_batch, void* d_pop,
                         const drl_replay* r, int64_t size, const uint8_t* d_double, hipStream_t stream) {
    drl::pop::Plan P;
    if (const char* msg = drl::pop::plan(d, members, max_batch, &P)) return fail(msg);
    drl::dd::PopArgs a;
    if (drl::pop::pop_train_args(&a, P, d_pop, r, size)) return -1;
    if (!d_double) return fail("d_double is NULL (a device array of `members` bytes: nonzero = Double DQN)");
    a.dbl = d_double;
    const int e = drl::dd::launch_pop_double_train(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_pop_double_train launch");
}

}  // extern "C"
