// dronerl_largelearn_api.cpp — C ABI of the large-batch DQN learner for dense nets (include/dronerl.h
// drl_dqn_large_*; kernels in dronerl_largelearn.hip, the agent block's layout in dronerl_largelearn_layout.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_internal.h"
#include "dronerl_largelearn_layout.h"

extern "C" __attribute__((visibility("hidden"))) int drl_internal_fail(const char* msg);

namespace {

int fail(const char* m) { return drl_internal_fail(m); }

int hip_fail(int e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString((hipError_t)e));
    return fail(buf);
}

// Every limit is checked here, by every call: nothing is refused at launch.
int ll_plan(const drl_qnet_desc* d, int32_t batch, drl::QnetLayout* L, drl::ll::Plan* P) {
    if (drl::qnet_layout_of(d, L)) return -1;
    const char* msg = drl::ll::plan(L->n_layers, L->in, L->out, L->code_w, batch, P);
    return msg ? fail(msg) : 0;
}

}  // namespace

// drl_dqn_large_train's checks behind its plan (a.P), then everything of the argument block but pack_status
int drl::ll::large_train_args(LearnArgs& a, int in_features, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                              const drl_replay* r, int64_t size) {
    const drl::ll::Plan& P = a.P;
    if (h->target_update_interval < 1 || h->epsilon_decay_every < 1)
        return fail("target_update_interval and epsilon_decay_every must be >= 1");
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0))
        return fail("beta1 and beta2 must be in [0, 1)");
    if (!d_agent || (uintptr_t)d_agent % 16) return fail("the agent block must be a 16-byte aligned device pointer");
    if (!d_packed || (uintptr_t)d_packed % 16) return fail("packed buffer must be a 16-byte aligned device pointer");
    if (!r || !r->obs || !r->next_obs || !r->actions || !r->rewards || !r->dones) return fail("replay buffers are NULL");
    if (r->capacity < 1 || r->capacity >= ((int64_t)1 << 31)) return fail("replay capacity must be in [1, 2^31)");
    if (size < 0 || size > r->capacity) return fail("size must be in [0, capacity]");
    if (P.code_w) {
        if ((int64_t)r->obs_floats * 4 != drl::lay::code_bytes(P.code_w))
            return fail("a DRL_QNET_INPUT_CODE net's replay rows are policy codes (drl_policy_code_bytes / 4 words)");
    } else if (r->obs_floats < in_features) {
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
    // the python floats as jax's weak typing rounds them into f32 arithmetic
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
    return 0;
}

extern "C" {

int drl_dqn_large_layout_query(const drl_qnet_desc* d, int32_t batch, drl_dqn_layout* layout) {
    drl::QnetLayout L;
    drl::ll::Plan P;
    if (ll_plan(d, batch, &L, &P)) return -1;
    if (!layout) return fail("layout is NULL");
    *layout = P.pub;
    return 0;
}

int drl_dqn_large_init(const drl_qnet_desc* d, int32_t batch, void* d_agent, float epsilon_start, hipStream_t stream) {
    drl::QnetLayout L;
    drl::ll::Plan P;
    if (ll_plan(d, batch, &L, &P)) return -1;
    if (!d_agent || (uintptr_t)d_agent % 16) return fail("the agent block must be a 16-byte aligned device pointer");
    uint8_t* base = static_cast<uint8_t*>(d_agent);
    // the moments; the init kernel sets the counters.  The scratch needs no clearing: every word a launch reads
    // was written by a launch before it in the same step.
    if (hipError_t e = hipMemsetAsync(base + P.pub.m_off, 0, (size_t)(P.pub.counters_off - P.pub.m_off), stream);
        e != hipSuccess)
        return hip_fail((int)e, "drl_dqn_large_init moments");
    hipError_t e = drl::launch_dqn_init(base + P.pub.counters_off, epsilon_start, stream);
    return e == hipSuccess ? 0 : hip_fail((int)e, "drl_dqn_large_init launch");
}

int drl_dqn_large_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
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
    const drl::ll::Plan& P = a.P;
    // the act's image of the new online set: the pack kernel itself on the online set, so the image is a fresh
    // drl_qnet_pack's byte for byte.  drl_qnet_pack clears the status vector with a hipMemsetAsync; here the
    // counters kernel stores the zeros instead, so that a captured call holds kernel nodes only.
    const float* w[drl::QN_MAX_LAYERS] = {};
    const float* b[drl::QN_MAX_LAYERS] = {};
    for (int l = 0; l < P.n_layers; ++l) {
        w[l] = a.online + P.woff[l];
        b[l] = a.online + P.boff[l];
    }
    drl::QnetPack pk;
    drl::qnet_pack_args(L, d_packed, w, b, &pk);
    a.pack_status = reinterpret_cast<uint32_t*>(pk.status);
    if (const int e = drl::ll::launch_large_train(a, stream); e != 0)
        return hip_fail(e, "drl_dqn_large_train launch");
    const hipError_t e = drl::launch_qnet_pack(pk, stream);
    return e == hipSuccess ? 0 : hip_fail((int)e, "drl_dqn_large_train pack launch");
}

int drl_dqn_large_sample_rows(const drl_qnet_desc* d, const drl_dqn_hparams* h, const void* d_agent, int64_t size,
                              int64_t* d_slots, hipStream_t stream) {
    drl::QnetLayout L;
    drl::ll::Plan P;
    if (!h) {
        if (ll_plan(d, 1, &L, &P)) return -1;
        return fail("hparams is NULL");
    }
    if (ll_plan(d, h->batch, &L, &P)) return -1;
    if (!d_agent || (uintptr_t)d_agent % 16) return fail("the agent block must be a 16-byte aligned device pointer");
    if (!d_slots || (uintptr_t)d_slots % 8) return fail("d_slots must be an 8-byte aligned device pointer");
    if (size < 1) return fail("size must be >= 1 (buffers.py can_sample: nothing is drawn from an empty ring)");
    const int e = drl::ll::launch_large_sample(static_cast<const uint8_t*>(d_agent) + P.pub.counters_off, h->sample_seed,
                                               h->batch, size, d_slots, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_dqn_large_sample_rows launch");
}

}  // extern "C"
