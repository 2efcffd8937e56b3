// dronerl_evalcode_api.cpp — C ABI of the multi-agent evaluator's kernels (include/dronerl.h drl_obs_code_all,
// drl_score_add; kernels in dronerl_evalcode.hip, geometry in dronerl_evalcode_layout.h).  Every argument is
// checked here, before any device work.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "dronerl_evalcode_layout.h"

using drl::fail;
using drl::hip_fail;

extern "C" {

int drl_obs_code_all(const drl_params* p, const drl_state* s, void* d_codes, hipStream_t stream) {
    drl_layout L;
    if (drl_layout_query(p, &L)) return -1;  // side, n_drones, window_radius, ... (names the failure)
    if (!s) return fail("drl_obs_code_all: state is NULL");
    if (s->num_envs <= 0) return fail("drl_obs_code_all: num_envs must be >= 1");
    if (!s->ground || !s->drones) return fail("drl_obs_code_all: state has NULL ground / drones");
    if ((uintptr_t)s->ground % 16 || (uintptr_t)s->drones % 4)
        return fail("drl_obs_code_all: ground must be 16-byte and drones 4-byte aligned");
    if (!d_codes) return fail("drl_obs_code_all: codes is NULL");
    if ((uintptr_t)d_codes % 16) return fail("drl_obs_code_all: codes must be 16-byte aligned");
    drl::ec::CodeAllArgs a;
    memset(&a, 0, sizeof a);
    a.g = drl::ec::geom_of(p->side, p->n_drones, p->window_radius);
    if (a.g.lds_bytes > drl::ec::kLdsBudget) return fail("drl_obs_code_all: one env's rows exceed the LDS budget");
    if ((s->num_envs + a.g.epw - 1) / a.g.epw > (int64_t)0x7fffffff) return fail("drl_obs_code_all: too many envs");
    a.E = s->num_envs;
    a.ground = s->ground;
    a.drones = s->drones;
    a.codes = static_cast<uint4*>(d_codes);
    const hipError_t e = drl::ec::launch_obs_code_all(a, stream);
    return e == hipSuccess ? 0 : hip_fail(e, "drl_obs_code_all launch");
}

int drl_score_add(const float* d_rewards, int64_t num_envs, int32_t n_drones, double crash_reward, double charge_reward,
                  double pickup_reward, double delivery_reward, double* d_scores, hipStream_t stream) {
    if (num_envs <= 0) return fail("drl_score_add: num_envs must be >= 1");
    if (n_drones < 1 || n_drones > DRL_MAX_DRONES) return fail("drl_score_add: n_drones outside [1, DRL_MAX_DRONES]");
    if (!d_rewards || !d_scores) return fail("drl_score_add: rewards / scores is NULL");
    if ((uintptr_t)d_rewards % 4 || (uintptr_t)d_scores % 8)
        return fail("drl_score_add: rewards must be 4-byte and scores 8-byte aligned");
    if (num_envs > ((int64_t)1 << 40) / n_drones) return fail("drl_score_add: too many envs");
    drl::ec::ScoreArgs a;
    a.rewards = d_rewards;
    a.scores = d_scores;
    a.n = num_envs * n_drones;
    a.v_crash = crash_reward;
    a.v_charge = charge_reward;
    a.v_pickup = pickup_reward;
    a.v_delivery = delivery_reward;
    a.f_crash = (float)crash_reward;
    a.f_charge = (float)charge_reward;
    a.f_pickup = (float)pickup_reward;
    a.f_delivery = (float)delivery_reward;
    const hipError_t e = drl::ec::launch_score_add(a, stream);
    return e == hipSuccess ? 0 : hip_fail(e, "drl_score_add launch");
}

}  // extern "C"
