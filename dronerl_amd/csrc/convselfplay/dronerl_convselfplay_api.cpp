// dronerl_convselfplay_api.cpp — C ABI of the conv learners' self-play act (include/dronerl.h
// drl_convselfplay_act; the kernel in dronerl_convselfplay.hip, the row map in dronerl_convselfplay_layout.h).
// The call validates its arguments before any device work and names the offending field through drl_last_error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "../dronerl_internal.h"
#include "dronerl_convselfplay_layout.h"

using drl::fail;
using drl::hip_fail;

extern "C" {

int drl_convselfplay_act(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                         const void* d_codes, int64_t num_envs, const int32_t* drones, int32_t team, int32_t greedy,
                         uint64_t seed, uint64_t step, int64_t env_offset, int32_t* d_actions, int32_t n_drones,
                         float* d_q, hipStream_t stream) {
    // drl_convleague_act's checks, with the map's (selfplay::check_map) behind the description's
    if (n_drones < 1 || n_drones > DRL_MAX_DRONES) return fail("n_drones must be in [1, 64]");
    const int32_t most = n_drones < DRL_POP_MAX_MEMBERS ? n_drones : DRL_POP_MAX_MEMBERS;
    if (members < 1 || members > most)
        return fail("members must be in [1, min(n_drones, DRL_POP_MAX_MEMBERS)]: every learner drives at least one drone");
    drl::cp::Plan P;
    if (const char* msg = drl::cp::plan(d, members, max_batch, &P)) return fail(msg);
    if (const char* msg = drl::selfplay::check_map(drones, members, team, n_drones)) return fail(msg);
    drl::cvl::ActPlan A;
    if (const char* msg = drl::cvl::act_plan(P, &A)) return fail(msg);
    if (!d_pop || (uintptr_t)d_pop % 16) return fail("the population block must be a 16-byte aligned device pointer");
    if (!d_codes || (uintptr_t)d_codes % 16)
        return fail("the policy codes must be a 16-byte aligned device pointer (drl_obs_code_all's output)");
    if (num_envs < 1 || num_envs * n_drones >= ((int64_t)1 << 31))
        return fail("num_envs must be >= 1 (and num_envs * n_drones < 2^31)");
    if ((int64_t)team * num_envs >= ((int64_t)1 << 31))
        return fail("team * num_envs (a learner's rows) must be < 2^31");
    if (!d_actions || (uintptr_t)d_actions % 4 || (uintptr_t)d_q % 4)
        return fail("actions must be non-NULL; actions and q 4-byte aligned");
    drl::cvs::ActArgs a;
    memset(&a, 0, sizeof a);
    a.c.P = P.P.c;
    a.c.A = A;
    a.c.members = members;
    a.c.stride = P.stride;
    a.c.base = static_cast<const uint8_t*>(d_pop);
    a.c.codes = static_cast<const uint32_t*>(d_codes);
    a.c.row_words = drl::lay::code_bytes(P.code_w) / 4;
    a.c.E = num_envs;
    a.c.greedy = greedy ? 1 : 0;
    a.c.n_drones = n_drones;
    a.c.seed = seed;
    a.c.step = step;
    a.c.env_offset = env_offset;
    a.c.actions = d_actions;
    a.c.q = d_q;
    a.team = team;
    a.rows = (int32_t)(team * num_envs);
    for (int e = 0; e < members * team; ++e) a.drones[e] = (uint8_t)drones[e];
    const int e = drl::cvs::launch_convselfplay_act(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convselfplay_act launch");
}

}  // extern "C"
