// dronerl_per_api.cpp — C ABI of the prioritized replay and its learner (include/dronerl.h drl_per_*,
// drl_dqn_per_train; kernels in dronerl_per.hip, the block's layout in dronerl_per_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "../largelearn/dronerl_largelearn_layout.h"
#include "dronerl_per_layout.h"

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
    if (!ph) return fail("the prioritized replay's hparams are NULL");
    if (!(ph->alpha >= 0.0)) return fail("alpha must be >= 0");
    if (!(ph->beta0 >= 0.0 && ph->beta0 <= 1.0)) return fail("beta0 must be in [0, 1]");
    if (ph->beta_steps < 0) return fail("beta_steps must be >= 0");
    if (!(ph->eps >= 0.0)) return fail("eps must be >= 0");
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
    drl::QnetLayout L;
    drl::per::LearnArgs a{};
    if (drl::qnet_layout_of(d, &L)) return -1;
    if (!h) return fail("hparams is NULL");
    if (const char* msg = drl::ll::plan(L.n_layers, L.in, L.out, L.code_w, h->batch, &a.P)) return fail(msg);
    const drl::ll::Plan& P = a.P;
    if (per_hparams(ph)) return -1;
    if (h->target_update_interval < 1 || h->epsilon_decay_every < 1)
        return fail("target_update_interval and epsilon_decay_every must be >= 1");
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0))
        return fail("beta1 and beta2 must be in [0, 1)");
    if (!d_agent || (uintptr_t)d_agent % 16) return fail("the agent block must be a 16-byte aligned device pointer");
    if (!d_packed || (uintptr_t)d_packed % 16) return fail("packed buffer must be a 16-byte aligned device pointer");
    if (!r || !r->obs || !r->next_obs || !r->actions || !r->rewards || !r->dones) return fail("replay buffers are NULL");
    drl::per::Plan T;
    if (per_block(r->capacity, h->batch, d_per, &T)) return -1;
    if (size < 0 || size > r->capacity) return fail("size must be in [0, capacity]");
    if (P.code_w) {
        if ((int64_t)r->obs_floats * 4 != drl::lay::code_bytes(P.code_w))
            return fail("a DRL_QNET_INPUT_CODE net's replay rows are policy codes (drl_policy_code_bytes / 4 words)");
    } else if (r->obs_floats < d->in_features) {
        return fail("replay obs_floats < in_features");
    }
    if ((uintptr_t)r->obs % 4 || (uintptr_t)r->next_obs % 4) return fail("replay rows must be 4-byte aligned");
    uint8_t* base = static_cast<uint8_t*>(d_agent);
    a.trained = size >= h->batch;  // buffers.py:92-93 can_sample
    a.code_w = P.code_w;
    a.online = reinterpret_cast<float*>(base + P.pub.online_off);
    a.target = reinterpret_cast<float*>(base + P.pub.target_off);
    a.adam_m = reinterpret_cast<float*>(base + P.pub.m_off);
    a.adam_v = reinterpret_cast<float*>(base + P.pub.v_off);
    a.ctr = reinterpret_cast<drl::DqnCounters*>(base + P.pub.counters_off);
    a.scratch = reinterpret_cast<float*>(base + P.pub.scratch_off);
    a.r_obs = reinterpret_cast<const uint32_t*>(r->obs);
    a.r_next = reinterpret_cast<const uint32_t*>(r->next_obs);
    a.row_words = r->obs_floats;
    a.r_act = r->actions;
    a.r_rew = r->rewards;
    a.r_done = r->dones;
    a.size = size;
    a.seed = h->sample_seed;
    // the python floats as jax's weak typing rounds them into f32 arithmetic (drl_dqn_large_train's)
    a.gamma = (float)h->gamma;
    a.b1 = (float)h->beta1;
    a.b2 = (float)h->beta2;
    a.c1 = (float)(1.0 - h->beta1);
    a.c2 = (float)(1.0 - h->beta2);
    a.adam_eps = (float)h->adam_eps;
    a.neg_lr = (float)(-h->learning_rate);
    a.tau = (float)h->tau;
    a.one_minus_tau = (float)(1.0 - h->tau);
    a.eps_decay = (float)h->epsilon_decay;
    a.eps_end = (float)h->epsilon_end;
    a.b1d = h->beta1;
    a.b2d = h->beta2;
    a.target_every = h->target_update_interval;
    a.eps_every = h->epsilon_decay_every;
    const drl::per::TreeArgs t = drl::per::tree_args(T, d_per);
    a.slots = t.slots;
    a.weights = t.weights;
    a.absd = t.absd;
    a.leaves = t.tree + t.P;
    a.pmax = t.pmax;
    a.alpha = ph->alpha;
    a.per_eps = ph->eps;
    const drl::per::SampleArgs sa = {h->sample_seed, size, ph->beta0, ph->beta_steps};
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

}  // extern "C"
