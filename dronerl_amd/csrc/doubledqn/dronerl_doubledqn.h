// dronerl_doubledqn.h — the Double DQN chains' kernel arguments and launches (kernels in dronerl_doubledqn.hip,
// launched by dronerl_doubledqn_api.cpp).  The argument blocks are the max-rule chains' own (ll::LearnArgs,
// per::LearnArgs, pop::PopArgs); the population adds the members' rule.
#ifndef DRONERL_DOUBLEDQN_H
#define DRONERL_DOUBLEDQN_H

#include <stdint.h>

#include "../largelearn/dronerl_largelearn_layout.h"
#include "../per/dronerl_per_layout.h"
#include "../population/dronerl_population_layout.h"

namespace drl {
namespace dd {

constexpr int kThreads = ll::kThreads;

// the population's arguments (the base: what the max-rule kernels of the chain are launched with) and the rule
struct PopArgs : pop::PopArgs {
    const uint8_t* dbl;  // DEVICE [members]: nonzero = the member's TD target is Double DQN's
};
static_assert(sizeof(PopArgs) <= 4096, "the arguments are read in place from the kernarg segment");

// (hipError_t values) one learner step's launches in stream order, without the pack: the max-rule chain's launch
// for launch, with this unit's forward (a third slice: the selector) and TD kernels in place of the chain's
int launch_double_train(const ll::LearnArgs& a, hipStream_t s);
int launch_double_per_train(const per::LearnArgs& a, const per::TreeArgs& t, const per::SampleArgs& sa, hipStream_t s);
int launch_pop_double_train(const PopArgs& a, hipStream_t s);

}  // namespace dd
}  // namespace drl
#endif
