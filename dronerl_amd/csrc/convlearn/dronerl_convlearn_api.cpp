// dronerl_convlearn_api.cpp — C ABI of the conv Q-network's learner (include/dronerl.h drl_convnet_dqn_*;
// kernels in dronerl_convlearn.hip, the agent block's layout in dronerl_convlearn_layout.h).  The calls are the
// shared front end's (../dronerl_learn_front.h) on the conv family.
#include "../dronerl_learn_front.h"

namespace front = drl::front;

extern "C" {

int drl_convnet_dqn_layout_query(const drl_convnet_desc* d, int32_t batch, drl_convnet_dqn_layout* layout) {
    return front::layout_query<front::Conv>(d, batch, layout);
}

int drl_convnet_dqn_init(const drl_convnet_desc* d, int32_t batch, void* d_agent, float epsilon_start,
                         hipStream_t stream) {
    return front::init<front::Conv>("drl_convnet_dqn_init", d, batch, d_agent, epsilon_start, stream);
}

// (A replayed graph's memset node was measured writing the first 16 bytes of another launch's arguments into the
// packed image's status vector when eager launches ran between the replays: hence the front end's pack without
// one)
int drl_convnet_dqn_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                          const drl_replay* r, int64_t size, hipStream_t stream) {
    return front::train<front::Conv, drl::cl::LearnArgs, front::NullHparams::kPlanAtBatch1>(
        "drl_convnet_dqn_train", d, h, nullptr, d_agent, d_packed, r, size, nullptr, stream,
        front::uniform<drl::cl::LearnArgs, drl::cl::launch_convnet_dqn_train>);
}

int drl_convnet_dqn_sample_rows(const drl_convnet_desc* d, const drl_dqn_hparams* h, const void* d_agent,
                                int64_t size, int64_t* d_slots, hipStream_t stream) {
    return front::sample_rows<front::Conv>("drl_convnet_dqn_sample_rows", d, h, d_agent, size, d_slots, stream);
}

}  // extern "C"
