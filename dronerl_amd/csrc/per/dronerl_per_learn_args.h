// dronerl_per_learn_args.h — a prioritized train call behind its plan (plain C++, no HIP call): the uniform
// call's checks (../dronerl_learn_args.h) in the prioritized calls' order, with the PER hyperparameters in front
// and the tree's plan, which refuses the ring's capacity here, behind the ring's pointers.  Dense, wide and conv,
// max-rule and Double: one order, so a bad argument is refused with the same message by each.
#ifndef DRONERL_PER_LEARN_ARGS_H
#define DRONERL_PER_LEARN_ARGS_H

#include <stdint.h>

#include "../dronerl_learn_args.h"
#include "dronerl_per_layout.h"

namespace drl {
namespace per {

// Every check of the hyperparameters, the blocks and the ring, then the chain's arguments (a.P is the caller's
// plan), the step's drawn rows (`d`, the chain's own member), the tree's view and the sampler's.  A refused call
// leaves all four as they were.
template <class A>
inline const char* learn_args(A& a, Drawn& d, int in_floats, const char* short_rows, const drl_dqn_hparams* h,
                              const drl_per_hparams* ph, void* d_agent, void* d_packed, const drl_replay* r,
                              int64_t size, void* d_per, TreeArgs* t, SampleArgs* sa) {
    if (const char* msg = check_hparams(ph)) return msg;
    if (const char* msg = check_learn_call(h, d_agent, d_packed, r, RingCapacity::kLeftToPerPlan)) return msg;
    Plan T;
    if (const char* msg = plan(r->capacity, h->batch, &T)) return msg;
    if (!d_per || (uintptr_t)d_per % 16) return "the prioritized replay block must be a 16-byte aligned device pointer";
    if (const char* msg = check_learn_size(r, size)) return msg;
    if (const char* msg = check_learn_rows(r, a.P.code_w, in_floats, short_rows)) return msg;
    fill_learn_args(a, a.P.pub, a.P.code_w, h, d_agent, r, size);
    *t = tree_args(T, d_per);
    d = drawn_of(*t, ph->alpha, ph->eps);
    *sa = SampleArgs{h->sample_seed, size, ph->beta0, ph->beta_steps};
    return nullptr;
}

}  // namespace per
}  // namespace drl
#endif
