// dronerl_per_learn_args.h — what the prioritized dense learners' train calls share on the host behind their
// plans (plain C++, no HIP): drl_dqn_per_train and drl_widenet_dqn_per_train (dronerl_per_api.cpp) and their
// Double DQN variants (doubledqn/dronerl_doubledqn_api.cpp) make the same checks in the same order, so a bad
// argument is refused with the same message by each.
#ifndef DRONERL_PER_LEARN_ARGS_H
#define DRONERL_PER_LEARN_ARGS_H

#include <stdint.h>

#include "../dronerl_learn_args.h"
#include "dronerl_per_layout.h"

namespace drl {
namespace per {

// Every check of the hyperparameters, the blocks and the ring, then the chain's arguments (a.P is the caller's
// plan), the tree's view and the sampler's.  Returns nullptr, or the message for drl_last_error.
inline const char* learn_args(LearnArgs& a, int in_features, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                              TreeArgs* t, SampleArgs* sa) {
    const ll::Plan& P = a.P;
    if (const char* msg = check_hparams(ph)) return msg;
    if (const char* msg = check_learn_call(h, d_agent, d_packed, r)) return msg;
    Plan T;
    if (const char* msg = plan(r->capacity, h->batch, &T)) return msg;
    if (!d_per || (uintptr_t)d_per % 16) return "the prioritized replay block must be a 16-byte aligned device pointer";
    if (size < 0 || size > r->capacity) return "size must be in [0, capacity]";
    if (const char* msg = check_learn_rows(r, P.code_w, in_features, "replay obs_floats < in_features")) return msg;
    fill_learn_args(a, P.pub, P.code_w, h, d_agent, r, size);
    *t = tree_args(T, d_per);
    a.d = drawn_of(*t, ph->alpha, ph->eps);
    *sa = SampleArgs{h->sample_seed, size, ph->beta0, ph->beta_steps};
    return nullptr;
}

}  // namespace per
}  // namespace drl
#endif
