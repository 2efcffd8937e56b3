// dronerl_learn_front.h — the host front end of the chain learners' C calls (the *_api.cpp units only): one
// description per net family, and layout_query, init, sample_rows and train written once over it.  A train call
// plans for the net at h->batch, checks the call and fills the chain's argument block (dronerl_learn_args.h;
// prioritized: per/dronerl_per_learn_args.h), builds the pack kernel's arguments on the new online set, then
// launches the chain and the pack.  Every limit is checked here, by every call: nothing is refused at launch.
#ifndef DRONERL_LEARN_FRONT_H
#define DRONERL_LEARN_FRONT_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/dronerl.h"
#include "dronerl_host.h"
#include "dronerl_internal.h"
#include "dronerl_learn_args.h"
#include "convper/dronerl_convper_layout.h"
#include "largelearn/dronerl_largelearn_layout.h"
#include "per/dronerl_per_learn_args.h"
#include "widenet/dronerl_widenet_layout.h"

namespace drl {
namespace front __attribute__((visibility("hidden"))) {  // (nothing of it is the library's to export)

// ---- the net families -------------------------------------------------------------------------------------------
// Desc: the net's description; Pub: the agent block's public layout; Plan: the learner's plan; Pack: the net's
// packed layout with the pack kernel's arguments.  layout/plan: 0, or -1 with the message set (plan = layout, then
// the learner's plan at `batch`).  pack_args: the act's image of the new online set, i.e. the family's pack kernel
// on the online set, so that the image is a fresh pack call's byte for byte; returns the image's status vector,
// which the chain's counters kernel clears in place of the pack call's hipMemsetAsync: a captured call then holds
// kernel nodes only.  (nullptr, with the message set: the description was refused.)

struct Dense {  // drl_qnet_desc: widths up to 128 (drl_dqn_large_*, drl_dqn_per_train, drl_dqn_double_*)
    using Desc = drl_qnet_desc;
    using Pub = drl_dqn_layout;
    using Plan = ll::Plan;
    struct Pack {
        QnetLayout L;
        QnetPack k;
    };
    static constexpr const char* kShortRows = kShortRowsDense;
    static constexpr const char* kInitClears = "moments";

    static int layout(const Desc* d, Pack* pk) { return qnet_layout_of(d, &pk->L); }
    static int plan(const Desc* d, int32_t batch, Pack* pk, Plan* P) {
        if (layout(d, pk)) return -1;
        const char* msg = ll::plan(pk->L.n_layers, pk->L.in, pk->L.out, pk->L.code_w, batch, P);
        return msg ? fail(msg) : 0;
    }
    static const Pub& pub(const Plan& P) { return P.pub; }
    static int in_floats(const Desc* d, const Plan&) { return d->in_features; }
    // the moments; the init kernel sets the counters.  The scratch needs no clearing: every word a launch reads
    // was written by a launch before it in the same step.
    static int64_t init_clear_end(const Pub& u) { return u.counters_off; }
    static int sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
        return ll::launch_large_sample(counters, seed, batch, size, out, s);
    }
    static uint32_t* pack_args(const Desc*, const Plan& P, const float* online, void* d_packed, Pack* pk) {
        const float* w[QN_MAX_LAYERS] = {};
        const float* b[QN_MAX_LAYERS] = {};
        for (int l = 0; l < P.n_layers; ++l) {
            w[l] = online + P.woff[l];
            b[l] = online + P.boff[l];
        }
        qnet_pack_args(pk->L, d_packed, w, b, &pk->k);
        return reinterpret_cast<uint32_t*>(pk->k.status);
    }
    static int launch_pack(const Pack& pk, hipStream_t s) { return (int)launch_qnet_pack(pk.k, s); }
};

struct Wide : Dense {  // drl_widenet_desc: the same chain on a plan with this family's width limit, its own pack
    using Desc = drl_widenet_desc;
    using Pack = wn::PackArgs;

    static int layout(const Desc* d, Pack* pk) {
        const char* msg = wn::layout(d, &pk->L);
        return msg ? fail(msg) : 0;
    }
    static int plan(const Desc* d, int32_t batch, Pack* pk, Plan* P) {
        if (layout(d, pk)) return -1;
        int32_t in[wn::kMaxLayers], out[wn::kMaxLayers];
        for (int l = 0; l < pk->L.n_layers; ++l) {
            in[l] = pk->L.l[l].in;
            out[l] = pk->L.l[l].out;
        }
        const char* msg = ll::plan(pk->L.n_layers, in, out, pk->L.code_w, batch, P, wn::kMaxWidth);
        return msg ? fail(msg) : 0;
    }
    static int in_floats(const Desc* d, const Plan&) { return d->in_features; }
    static uint32_t* pack_args(const Desc*, const Plan& P, const float* online, void* d_packed, Pack* pk) {
        for (int l = 0; l < P.n_layers; ++l) {
            pk->w[l] = online + P.woff[l];
            pk->b[l] = online + P.boff[l];
        }
        pk->packed = static_cast<uint32_t*>(d_packed);
        return pk->packed + pk->L.status;
    }
    static int launch_pack(const Pack& pk, hipStream_t s) { return wn::launch_widenet_pack(pk, s); }
};

struct Conv {  // drl_convnet_desc at batches up to 64 (drl_convnet_dqn_*)
    using Desc = drl_convnet_desc;
    using Pub = drl_convnet_dqn_layout;
    using Plan = cl::Plan;
    using Pack = cv::PackArgs;  // (its layout is made with the pack's arguments: the plan validates the net)
    static constexpr const char* kShortRows = kShortRowsConv;
    static constexpr const char* kInitClears = "moments, counters and scratch";

    static int plan(const Desc* d, int32_t batch, Pack*, Plan* P) {
        const char* msg = cl::plan(d, batch, P);
        return msg ? fail(msg) : 0;
    }
    static const Pub& pub(const Plan& P) { return P.pub; }
    static int in_floats(const Desc*, const Plan& P) { return P.in; }
    // the moments, and the counters with the scratch behind them (the init kernel then sets the counters)
    static int64_t init_clear_end(const Pub& u) { return u.bytes; }
    static int sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
        return (int)launch_dqn_sample(counters, seed, batch, size, out, s);
    }
    static uint32_t* pack_args(const Desc* d, const cl::Plan& P, const float* online, void* d_packed, Pack* pk) {
        if (const char* msg = cv::layout(d, &pk->L)) {
            fail(msg);
            return nullptr;
        }
        for (int l = 0; l < P.n_layers; ++l) {
            pk->w[l] = online + P.l[l].woff;
            pk->b[l] = online + P.l[l].boff;
        }
        pk->packed = static_cast<uint32_t*>(d_packed);
        return pk->packed + pk->L.status;
    }
    static int launch_pack(const Pack& pk, hipStream_t s) { return cv::launch_convnet_pack(pk, s); }
};

struct ConvLarge : Conv {  // ... at batches up to 4096 (drl_convnet_dqn_large_*, drl_convnet_dqn_per_train)
    using Plan = cg::Plan;
    static constexpr const char* kInitClears = "moments and counters";

    static int plan(const Desc* d, int32_t batch, Pack*, Plan* P) {
        const char* msg = cg::plan(d, batch, P);
        return msg ? fail(msg) : 0;
    }
    static const Pub& pub(const Plan& P) { return P.c.pub; }
    static int in_floats(const Desc*, const Plan& P) { return P.c.in; }
    // the moments and the counters (the init kernel then sets the counters); the scratch needs no clearing: a
    // step writes every word of it that it reads
    static int64_t init_clear_end(const Pub& u) { return u.scratch_off; }
    static int sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s) {
        return cg::launch_convlarge_sample(counters, seed, batch, size, out, s);
    }
};

// ---- a chain's argument block: the learner view in it that the checks fill, with the plan put in -------------------
inline ll::LearnArgs& learner_of(ll::LearnArgs& a, const ll::Plan& P) {  // (per::LearnArgs derives from it)
    a.P = P;
    return a;
}
inline cl::LearnArgs& learner_of(cl::LearnArgs& a, const cl::Plan& P) {
    a.P = P;
    return a;
}
inline cl::LearnArgs& learner_of(cg::LearnArgs& a, const cg::Plan& P) {
    a.t = P.t;
    return learner_of(a.a, P.c);
}
inline cl::LearnArgs& learner_of(cper::LearnArgs& a, const cg::Plan& P) { return learner_of(a.c, P); }

// the prioritized chains' blocks hold the step's drawn rows as `d`
template <class Args>
constexpr bool kPrioritized = std::is_same<Args, per::LearnArgs>::value || std::is_same<Args, cper::LearnArgs>::value;

// A call without hyperparameters is refused for a bad description first.  The calls differ in how far that check
// goes, and keep their difference: the uniform calls (and the conv prioritized one) make the whole plan at batch
// 1, the dense and wide prioritized calls the net's layout alone (so a net whose plan alone is refused is told
// "hparams is NULL" by these).
enum class NullHparams { kPlanAtBatch1, kLayoutOnly };

// a uniform chain as train's launcher: the tree and the sampler are not its to read
template <class Args, int (*kLaunch)(const Args&, hipStream_t)>
int uniform(const Args& a, const per::TreeArgs&, const per::SampleArgs&, hipStream_t s) {
    return kLaunch(a, s);
}

inline int launch_fail(int e, const char* call, const char* step) {
    char what[128];
    snprintf(what, sizeof what, "%s %s", call, step);
    return hip_fail(e, what);
}

// ---- the calls --------------------------------------------------------------------------------------------------
template <class F>
int layout_query(const typename F::Desc* d, int32_t batch, typename F::Pub* layout) {
    typename F::Pack pk;
    typename F::Plan P;
    if (F::plan(d, batch, &pk, &P)) return -1;
    if (!layout) return fail("layout is NULL");
    *layout = F::pub(P);
    return 0;
}

template <class F>
int init(const char* call, const typename F::Desc* d, int32_t batch, void* d_agent, float epsilon_start,
         hipStream_t stream) {
    typename F::Pack pk;
    typename F::Plan P;
    if (F::plan(d, batch, &pk, &P)) return -1;
    if (const char* msg = check_agent_block(d_agent)) return fail(msg);
    uint8_t* base = static_cast<uint8_t*>(d_agent);
    const typename F::Pub& u = F::pub(P);
    if (hipError_t e = hipMemsetAsync(base + u.m_off, 0, (size_t)(F::init_clear_end(u) - u.m_off), stream);
        e != hipSuccess)
        return launch_fail((int)e, call, F::kInitClears);
    const hipError_t e = launch_dqn_init(base + u.counters_off, epsilon_start, stream);
    return e == hipSuccess ? 0 : launch_fail((int)e, call, "launch");
}

template <class F>
int sample_rows(const char* call, const typename F::Desc* d, const drl_dqn_hparams* h, const void* d_agent,
                int64_t size, int64_t* d_slots, hipStream_t stream) {
    typename F::Pack pk;
    typename F::Plan P;
    if (F::plan(d, h ? h->batch : 1, &pk, &P)) return -1;
    if (!h) return fail("hparams is NULL");
    if (const char* msg = check_agent_block(d_agent)) return fail(msg);
    if (!d_slots || (uintptr_t)d_slots % 8) return fail("d_slots must be an 8-byte aligned device pointer");
    if (size < 1) return fail("size must be >= 1 (buffers.py can_sample: nothing is drawn from an empty ring)");
    const int e = F::sample(static_cast<const uint8_t*>(d_agent) + F::pub(P).counters_off, h->sample_seed, h->batch,
                            size, d_slots, stream);
    return e == 0 ? 0 : launch_fail(e, call, "launch");
}

// One learner step.  Args: the chain's argument block (prioritized iff it holds drawn rows; ph and d_per are
// theirs, NULL in a uniform call).  launch(args, tree, sampler, stream): the chain, uniform, prioritized or
// Double; a uniform one ignores the tree and the sampler.
template <class F, class Args, NullHparams kNullH, class Launch>
int train(const char* call, const typename F::Desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
          void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per, hipStream_t stream,
          Launch launch) {
    typename F::Pack pk;
    memset(&pk, 0, sizeof pk);
    typename F::Plan P;
    if constexpr (kNullH == NullHparams::kLayoutOnly) {
        if (!h) return F::layout(d, &pk) ? -1 : fail("hparams is NULL");
    }
    if (F::plan(d, h ? h->batch : 1, &pk, &P)) return -1;
    if (!h) return fail("hparams is NULL");
    Args args;
    memset(&args, 0, sizeof args);
    auto& a = learner_of(args, P);
    per::TreeArgs t{};
    per::SampleArgs sa{};
    const char* msg;
    if constexpr (kPrioritized<Args>)
        msg = per::learn_args(a, args.d, F::in_floats(d, P), F::kShortRows, h, ph, d_agent, d_packed, r, size, d_per,
                              &t, &sa);
    else
        msg = learn_args(a, F::in_floats(d, P), F::kShortRows, h, d_agent, d_packed, r, size);
    if (msg) return fail(msg);
    a.pack_status = F::pack_args(d, a.P, a.online, d_packed, &pk);
    if (!a.pack_status) return -1;
    if (const int e = launch(args, t, sa, stream); e != 0) return launch_fail(e, call, "launch");
    const int e = F::launch_pack(pk, stream);
    return e == 0 ? 0 : launch_fail(e, call, "pack launch");
}

}  // namespace front
}  // namespace drl
#endif
