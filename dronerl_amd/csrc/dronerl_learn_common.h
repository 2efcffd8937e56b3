// dronerl_learn_common.h — device code shared by the DQN learners (dronerl_learn.hip, the dense nets' single
// launch; convlearn/dronerl_convlearn.hip, the conv nets' launch chain), in the manner of dronerl_act_common.h:
// the replay row draw, the launch chains' policy of how a row is drawn and weighted (uniform or prioritized), a
// row's input decode, optax's Adam and incremental_update, and the counters at the end of a step.  Every learner
// includes it, so they cannot drift apart on the sample hash, the TD rule's weighting, the Adam formula or the
// epsilon schedule.  The functions take the learner's own argument block (any struct with the fields they
// name): the dense learner's LearnArgs, the conv learner's cl::LearnArgs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronerl_internal.h"
#include "dronerl_act_common.h"

// every product and sum rounds on its own (no FMA contraction): the order oracle/dqn_learner.py restates
#pragma clang fp contract(off)

namespace drl {

// buffers.py:79-90: B uniform indices in [0, current_size) (the reference draws
// them with jax.random.randint; here a counter hash of (seed, step, row)).
__device__ __forceinline__ int64_t dq_sample(uint64_t seed, int32_t step, int b, int64_t size) {
    const uint64_t h = splitmix64(seed ^ splitmix64(((uint64_t)(uint32_t)step << 16) | (uint64_t)b));
    return (int64_t)(((h >> 32) * (uint64_t)size) >> 32);
}

// How a launch chain's row b is drawn and weighted: the one thing in which a uniform chain and a prioritized one
// differ.  The chains' rows and TD bodies take the policy as `p` and are compiled once for each:
//   UniformRows     the slot is dq_sample's; no weight; nothing is kept.
//   a drawn view    (any struct with per::Drawn's fields, per/dronerl_per_layout.h) the slot and the importance
//                   weight are the sampler's; the weight lies on the row's squared error and on the Q head's
//                   delta; |d| is kept for the priority kernel and the slot's leaf zeroed, so that the integer
//                   max there starts from 0.0 (a slot drawn by several rows is zeroed by each: the same store).
// The choice is the overload's, at compile time: the uniform kernels hold no weight load and no multiply.
struct UniformRows {};

// Row b's slot.  The arguments are dq_sample's, which a drawn row leaves unread: each body names them in the order
// in which it has always read them.
__device__ __forceinline__ int64_t dq_row_slot(const UniformRows&, uint64_t seed, int32_t step, int b, int64_t size) {
    return dq_sample(seed, step, b, size);
}
template <class Drawn>
__device__ __forceinline__ int64_t dq_row_slot(const Drawn& p, uint64_t, int32_t, int b, int64_t) {
    return p.slots[b];
}

// Row b's importance weight, read once, and a term x of the row's loss under it: the uniform case has no weight
// to read and x stays as it is (no multiply by 1.0)
struct Unweighted {};
__device__ __forceinline__ Unweighted dq_row_weight(const UniformRows&, int) { return Unweighted{}; }
template <class Drawn>
__device__ __forceinline__ float dq_row_weight(const Drawn& p, int b) {
    return p.weights[b];
}
__device__ __forceinline__ float dq_weighted(Unweighted, float x) { return x; }
__device__ __forceinline__ float dq_weighted(float w, float x) { return w * x; }

// What is kept of row b (replay slot s) once its TD error d is known.  A body that does not hold the slot leaves
// it out: a drawn row's is read again, a uniform row's never computed.
__device__ __forceinline__ void dq_row_keep(const UniformRows&, int, int64_t, float) {}
__device__ __forceinline__ void dq_row_keep(const UniformRows&, int, float) {}
template <class Drawn>
__device__ __forceinline__ void dq_row_keep(const Drawn& p, int b, int64_t s, float d) {
    p.absd[b] = __builtin_fabsf(d);
    p.leaves[s] = 0.0f;
}
template <class Drawn>
__device__ __forceinline__ void dq_row_keep(const Drawn& p, int b, float d) {
    dq_row_keep(p, b, p.slots[b], d);
}

// The target rule: which of the target net's next-state values a row's TD target takes.  The second compile-time
// policy of the launch chains' TD body, next to the rows' policy:
//   MaxTarget       max_a Q_target(next_obs) (dqn.py:160-167; jnp.max).  The selector's values are never read.
//   DoubleTarget    Q_target(next_obs)[a*], a* = argmax_a Q_online(next_obs) (van Hasselt et al. 2016): the first
//                   maximum, as jnp.argmax; a NaN never wins a comparison.  The selection is an index: no gradient
//                   flows through the selector's values.
// qt, qs: the target's and the selector's Q values of the row, A of them (A <= kTargetRuleActions).
struct MaxTarget {};
struct DoubleTarget {};
constexpr int kTargetRuleActions = 8;  // drl_qnet_desc's limit on n_actions

__device__ __forceinline__ float dq_next_value(const MaxTarget&, const float* qt, const float*, int A) {
    float mx = qt[0];
    for (int j = 1; j < A; ++j) mx = qt[j] > mx ? qt[j] : mx;  // jnp.max
    return mx;
}
__device__ __forceinline__ float dq_next_value(const DoubleTarget&, const float* qt, const float* qs, int A) {
    // a* = 0; for j = 1 .. A-1: if qs[j] > qs[a*]: a* = j -- with qs[a*] and qt[a*] carried instead of the index
    float best = qs[0], v = qt[0];
#pragma unroll
    for (int j = 1; j < kTargetRuleActions; ++j)
        if (j < A && qs[j] > best) {
            best = qs[j];
            v = qt[j];
        }
    return v;
}

// The selector's Q values of a row, read into registers (qs) from the words `from` before anything overwrites
// them; the max rule has none to read.
__device__ __forceinline__ void dq_selector_values(const MaxTarget&, float*, const float*, int) {}
__device__ __forceinline__ void dq_selector_values(const DoubleTarget&, float* qs, const float* from, int A) {
#pragma unroll
    for (int j = 0; j < kTargetRuleActions; ++j) qs[j] = j < A ? from[j] : 0.0f;
}

// Input k of replay row s: a policy-code row is decoded with the channel rules
// of the observation writer (wrappers.py:10-31; drl_code_decode), an f32 row read.
template <class Args>
__device__ __forceinline__ float dq_input(const Args& a, const uint32_t* __restrict__ rows, int64_t s, int k) {
    const uint32_t* row = rows + s * a.row_words;
    if (a.code_w == 0) return __uint_as_float(row[k]);
    const int cpg = lay::code_cpg(a.code_w), cpg8 = lay::code_cpg8(a.code_w);
    const int cl = k / 6, ch = k - 6 * cl, grp = cl / cpg;
    const uint32_t h = reinterpret_cast<const uint16_t*>(row)[grp * cpg8 + (cl - grp * cpg)];
    const uint32_t obj = h & 7u, air = h >> 3;
    switch (ch) {
        case 0: return air ? 1.0f : 0.0f;
        case 1: return (obj == OBJ_PACKET || (air & 0x80u)) ? 1.0f : 0.0f;
        case 2: return obj == OBJ_DROPZONE ? 1.0f : 0.0f;
        case 3: return obj == OBJ_STATION ? 1.0f : 0.0f;
        case 4: return air ? (float)((int)(air & 0x7fu) - 1) / 100.0f : 0.0f;
        default: return obj == OBJ_SKYSCRAPER ? 1.0f : 0.0f;
    }
}

// optax.adam (scale_by_adam + scale(-lr)) + apply_updates, term by term:
// mu = (1-b1) g + b1 mu; nu = (1-b2) g^2 + b2 nu; u = (mu / bc1) / (sqrt(nu / bc2)
// + eps); p + u * (-lr).
template <class Args>
__device__ __forceinline__ float dq_adam(const Args& a, float p, float g, float* __restrict__ m,
                                         float* __restrict__ v, float bc1, float bc2) {
    const float mn = a.c1 * g + a.b1 * *m;
    const float vn = a.c2 * (g * g) + a.b2 * *v;
    *m = mn;
    *v = vn;
    const float u = (mn / bc1) / (__builtin_sqrtf(vn / bc2) + a.adam_eps);
    return p + u * a.neg_lr;
}

// optax.incremental_update(new, old, tau) = tau * new + (1 - tau) * old
template <class Args>
__device__ __forceinline__ float dq_blend(const Args& a, float nw, float old) {
    return a.tau * nw + a.one_minus_tau * old;
}

// The counters at the end of a learner step (one thread): Adam's count and
// powers, the loss, the epsilon decay, the step's plan (informative),
// step + 1.  ctr: the values the step read at its start.
template <class Args>
__device__ __forceinline__ void dq_finish_counters(const Args& a, DqnCounters* c, const DqnCounters& ctr, int trained,
                                                   float loss, float bc1, float bc2) {
    const int32_t step = ctr.step;
    if (trained) {
        c->count = ctr.count + 1;
        c->beta1_pow = ctr.beta1_pow * a.b1d;
        c->beta2_pow = ctr.beta2_pow * a.b2d;
    }
    c->loss = trained ? loss : 0.0f;
    float eps = ctr.epsilon;
    if (step % a.eps_every == 0) {
        const float d = eps * a.eps_decay;
        eps = d > a.eps_end ? d : a.eps_end;  // jnp.maximum
    }
    c->epsilon = eps;
    c->trained = trained;
    c->target_due = step % a.target_every == 0 ? 1 : 0;
    c->bc1 = bc1;
    c->bc2 = bc2;
    c->step = step + 1;
}

}  // namespace drl
