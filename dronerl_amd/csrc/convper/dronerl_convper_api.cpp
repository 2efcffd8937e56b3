// dronerl_convper_api.cpp — C ABI of the prioritized conv learner (include/dronerl.h drl_convnet_dqn_per_train;
// kernels in dronerl_convper.hip).  The call is the shared front end's (../dronerl_learn_front.h): the agent
// block and its plan are drl_convnet_dqn_large_train's (convlarge/), the prioritized block and the order of the
// checks drl_dqn_per_train's (per/).
#include "../dronerl_learn_front.h"

namespace front = drl::front;

extern "C" {

// (Unlike the dense prioritized calls, this one makes its whole plan at batch 1 before it refuses NULL hparams.)
int drl_convnet_dqn_per_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const drl_replay* r, int64_t size, void* d_per,
                              hipStream_t stream) {
    return front::train<front::ConvLarge, drl::cper::LearnArgs, front::NullHparams::kPlanAtBatch1>(
        "drl_convnet_dqn_per_train", d, h, ph, d_agent, d_packed, r, size, d_per, stream,
        drl::cper::launch_convper_train);
}

}  // extern "C"
