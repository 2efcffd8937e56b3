// dronerl_doubledqn_api.cpp — C ABI of the Double DQN learner calls (include/dronerl.h drl_dqn_double_train,
// drl_widenet_dqn_double_train, drl_dqn_double_per_train, drl_widenet_dqn_double_per_train, drl_pop_double_train;
// kernels in dronerl_doubledqn.hip).  Each single-agent call is its max-rule call (the shared front end,
// ../dronerl_learn_front.h, on the same family with the same order of checks) with the Double chain for a launcher;
// drl_pop_double_train makes drl_pop_train's checks through pop::pop_train_args.
#include "../dronerl_learn_front.h"
#include "../population/dronerl_population_layout.h"
#include "dronerl_doubledqn.h"

namespace front = drl::front;
using drl::fail;
using drl::hip_fail;

extern "C" {

int drl_dqn_double_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                         const drl_replay* r, int64_t size, hipStream_t stream) {
    return front::train<front::Dense, drl::ll::LearnArgs, front::NullHparams::kPlanAtBatch1>(
        "drl_dqn_double_train", d, h, nullptr, d_agent, d_packed, r, size, nullptr, stream,
        front::uniform<drl::ll::LearnArgs, drl::dd::launch_double_train>);
}

int drl_widenet_dqn_double_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                                 const drl_replay* r, int64_t size, hipStream_t stream) {
    return front::train<front::Wide, drl::ll::LearnArgs, front::NullHparams::kPlanAtBatch1>(
        "drl_widenet_dqn_double_train", d, h, nullptr, d_agent, d_packed, r, size, nullptr, stream,
        front::uniform<drl::ll::LearnArgs, drl::dd::launch_double_train>);
}

int drl_dqn_double_per_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                             void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                             hipStream_t stream) {
    return front::train<front::Dense, drl::per::LearnArgs, front::NullHparams::kLayoutOnly>(
        "drl_dqn_double_per_train", d, h, ph, d_agent, d_packed, r, size, d_per, stream,
        drl::dd::launch_double_per_train);
}

int drl_widenet_dqn_double_per_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                                     void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                                     hipStream_t stream) {
    return front::train<front::Wide, drl::per::LearnArgs, front::NullHparams::kLayoutOnly>(
        "drl_widenet_dqn_double_per_train", d, h, ph, d_agent, d_packed, r, size, d_per, stream,
        drl::dd::launch_double_per_train);
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
