// dronerl_convper_layout.h — the arguments of the prioritized conv learner's launch chain (include/dronerl.h
// drl_convnet_dqn_per_train).  There is no new block: the agent block is the conv large-batch learner's
// (convlarge/dronerl_convlarge_layout.h), the prioritized block the dense learner's (per/dronerl_per_layout.h).
// Plain C++ (no HIP): the host API and the kernels share it.
#ifndef DRONERL_CONVPER_LAYOUT_H
#define DRONERL_CONVPER_LAYOUT_H

#include <stdint.h>

#include "../convlarge/dronerl_convlarge_layout.h"
#include "../per/dronerl_per_layout.h"

namespace drl {
namespace cper {

static_assert(per::kMaxBatch == cg::kMaxBatch, "one prioritized block serves both learners' batches");

// the conv large-batch chain's arguments and the step's drawn rows
struct LearnArgs {
    cg::LearnArgs c;  // (c.a is the agent view the chain's bodies take, c.t the chain's tiles; the uniform
                      // kernels of the chain are launched with c)
    per::Drawn d;
};
static_assert(sizeof(LearnArgs) <= 4096, "the arguments are read in place from the kernarg segment");

// (hipError_t values) one learner step without the pack: rebuild, sample, the chain with the priority update
// (c.a.trained), or the chain's no-sample step
int launch_convper_train(const LearnArgs& a, const per::TreeArgs& t, const per::SampleArgs& sa, hipStream_t s);

}  // namespace cper
}  // namespace drl
#endif
