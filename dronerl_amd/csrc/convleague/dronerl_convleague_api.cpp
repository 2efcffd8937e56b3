// dronerl_convleague_api.cpp — C ABI of the conv league's act (include/dronerl.h drl_convleague_*; the kernel in
// dronerl_convleague.hip, the plan in dronerl_convleague_layout.h).  Every call validates its arguments before
// any device work and names the offending field through drl_last_error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "../dronerl_internal.h"
#include "dronerl_convleague_layout.h"

using drl::fail;
using drl::hip_fail;

extern "C" {

int drl_convleague_act_plan_query(const drl_convnet_desc* d, drl_convleague_act_plan* plan) {
    drl::cp::Plan P;
    const char* msg = drl::cp::plan(d, 1, 1, &P);
    if (msg) return fail(msg);
    if (!plan) return fail("plan is NULL");
    drl::cvl::ActPlan A;
    if ((msg = drl::cvl::act_plan(P, &A))) return fail(msg);
    memset(plan, 0, sizeof *plan);
    plan->env_tile = A.env_tile;
    plan->threads = A.threads;
    plan->row_words = A.row_words;
    plan->lds_bytes = A.lds_bytes;
    plan->lds_limit = drl::cvl::kLdsLimit;
    return 0;
}

int drl_convleague_act(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                       const void* d_codes, int64_t num_envs, int32_t greedy, uint64_t seed, uint64_t step,
                       int64_t env_offset, int32_t* d_actions, int32_t n_drones, float* d_q, hipStream_t stream) {
    if (n_drones < 1 || n_drones > DRL_MAX_DRONES) return fail("n_drones must be in [1, 64]");
    const int32_t most = n_drones < DRL_POP_MAX_MEMBERS ? n_drones : DRL_POP_MAX_MEMBERS;
    if (members < 1 || members > most)
        return fail("members must be in [1, min(n_drones, DRL_POP_MAX_MEMBERS)]: learner k drives drone index k");
    drl::cp::Plan P;
    if (const char* msg = drl::cp::plan(d, members, max_batch, &P)) return fail(msg);
    drl::cvl::ActPlan A;
    if (const char* msg = drl::cvl::act_plan(P, &A)) return fail(msg);
    if (!d_pop || (uintptr_t)d_pop % 16) return fail("the population block must be a 16-byte aligned device pointer");
    if (!d_codes || (uintptr_t)d_codes % 16)
        return fail("the policy codes must be a 16-byte aligned device pointer (drl_obs_code_all's output)");
    if (num_envs < 1 || num_envs * n_drones >= ((int64_t)1 << 31))
        return fail("num_envs must be >= 1 (and num_envs * n_drones < 2^31)");
    if (!d_actions || (uintptr_t)d_actions % 4 || (uintptr_t)d_q % 4)
        return fail("actions must be non-NULL; actions and q 4-byte aligned");
    drl::cvl::ActArgs a;
    memset(&a, 0, sizeof a);
    a.P = P.P.c;
    a.A = A;
    a.members = members;
    a.stride = P.stride;
    a.base = static_cast<const uint8_t*>(d_pop);
    a.codes = static_cast<const uint32_t*>(d_codes);
    a.row_words = drl::lay::code_bytes(P.code_w) / 4;
    a.E = num_envs;
    a.greedy = greedy ? 1 : 0;
    a.n_drones = n_drones;
    a.seed = seed;
    a.step = step;
    a.env_offset = env_offset;
    a.actions = d_actions;
    a.q = d_q;
    const int e = drl::cvl::launch_convleague_act(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convleague_act launch");
}

}  // extern "C"
