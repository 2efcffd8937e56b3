// dronerl_largelearn_api.cpp — C ABI of the large-batch DQN learner for dense nets (include/dronerl.h
// drl_dqn_large_*; kernels in dronerl_largelearn.hip, the agent block's layout in dronerl_largelearn_layout.h).
// The calls are the shared front end's (../dronerl_learn_front.h) on the dense family.
#include "../dronerl_learn_front.h"

namespace front = drl::front;

extern "C" {

int drl_dqn_large_layout_query(const drl_qnet_desc* d, int32_t batch, drl_dqn_layout* layout) {
    return front::layout_query<front::Dense>(d, batch, layout);
}

int drl_dqn_large_init(const drl_qnet_desc* d, int32_t batch, void* d_agent, float epsilon_start, hipStream_t stream) {
    return front::init<front::Dense>("drl_dqn_large_init", d, batch, d_agent, epsilon_start, stream);
}

int drl_dqn_large_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                        const drl_replay* r, int64_t size, hipStream_t stream) {
    return front::train<front::Dense, drl::ll::LearnArgs, front::NullHparams::kPlanAtBatch1>(
        "drl_dqn_large_train", d, h, nullptr, d_agent, d_packed, r, size, nullptr, stream,
        front::uniform<drl::ll::LearnArgs, drl::ll::launch_large_train>);
}

int drl_dqn_large_sample_rows(const drl_qnet_desc* d, const drl_dqn_hparams* h, const void* d_agent, int64_t size,
                              int64_t* d_slots, hipStream_t stream) {
    return front::sample_rows<front::Dense>("drl_dqn_large_sample_rows", d, h, d_agent, size, d_slots, stream);
}

}  // extern "C"
