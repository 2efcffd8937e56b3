// dronerl_league_api.cpp — C ABI of the league (include/dronerl.h drl_league_*; kernels in dronerl_league.hip,
// the plan in dronerl_league_layout.h).  Every call validates its arguments before any device work and names the
// offending field through drl_last_error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_args.h"
#include "dronerl_league_layout.h"

using drl::fail;
using drl::hip_fail;

namespace {

// The description, the league's size and the drones: every limit is checked here, by every call.
int league_plan(const drl_widenet_desc* d, int32_t members, int32_t max_batch, int32_t n_drones, drl::pop::Plan* P) {
    if (n_drones < 1 || n_drones > DRL_MAX_DRONES) return fail("n_drones must be in [1, 64]");
    const int32_t most = n_drones < DRL_POP_MAX_MEMBERS ? n_drones : DRL_POP_MAX_MEMBERS;
    if (members < 1 || members > most)
        return fail("members must be in [1, min(n_drones, DRL_POP_MAX_MEMBERS)]: learner k drives drone index k");
    const char* msg = drl::pop::plan(d, members, max_batch, P);
    return msg ? fail(msg) : 0;
}

int check_codes(const void* p, const char* what) {
    if (!p || (uintptr_t)p % 16) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s must be a 16-byte aligned device pointer (drl_obs_code_all's output)", what);
        return fail(buf);
    }
    return 0;
}

}  // namespace

extern "C" {

int drl_league_act_plan_query(const drl_widenet_desc* d, drl_league_act_plan* plan) {
    drl::pop::Plan P;
    const char* msg = drl::pop::plan(d, 1, 1, &P);
    if (msg) return fail(msg);
    if (!plan) return fail("plan is NULL");
    drl::league::ActPlan A;
    if ((msg = drl::league::act_plan(P, &A))) return fail(msg);
    memset(plan, 0, sizeof *plan);
    plan->env_tile = drl::league::kEnvTile;
    plan->threads = drl::league::kActThreads;
    plan->pass_units = drl::league::kPassUnits;
    plan->chunk_k = drl::league::kChunkK;
    plan->ldx = A.ldx;
    plan->lda = A.lda;
    plan->lds_bytes = A.lds_bytes;
    plan->lds_limit = drl::league::kLdsLimit;
    return 0;
}

int drl_league_act(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                   const void* d_codes, int64_t num_envs, int32_t greedy, uint64_t seed, uint64_t step,
                   int64_t env_offset, int32_t* d_actions, int32_t n_drones, float* d_q, hipStream_t stream) {
    drl::pop::Plan P;
    if (league_plan(d, members, max_batch, n_drones, &P)) return -1;
    drl::league::ActPlan A;
    if (const char* msg = drl::league::act_plan(P, &A)) return fail(msg);
    if (!d_pop || (uintptr_t)d_pop % 16) return fail("the population block must be a 16-byte aligned device pointer");
    if (check_codes(d_codes, "the policy codes")) return -1;
    if (num_envs < 1 || num_envs * n_drones >= ((int64_t)1 << 31))
        return fail("num_envs must be >= 1 (and num_envs * n_drones < 2^31)");
    if (!d_actions || (uintptr_t)d_actions % 4 || (uintptr_t)d_q % 4)
        return fail("actions must be non-NULL; actions and q 4-byte aligned");
    drl::league::ActArgs a;
    memset(&a, 0, sizeof a);
    a.P = P.P;
    a.A = A;
    a.members = members;
    a.n_actions = P.n_actions;
    a.stride = P.stride;
    a.base = static_cast<const uint8_t*>(d_pop);
    a.codes = static_cast<const uint32_t*>(d_codes);
    a.row_words = drl::lay::code_bytes(P.P.code_w) / 4;
    if (a.row_words != drl::league::code_row_words(P.P.code_w)) return fail("internal: the league plan's code row differs from the env's");
    a.E = num_envs;
    a.greedy = greedy ? 1 : 0;
    a.n_drones = n_drones;
    a.seed = seed;
    a.step = step;
    a.env_offset = env_offset;
    a.actions = d_actions;
    a.q = d_q;
    const int e = drl::league::launch_league_act(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_league_act launch");
}

int drl_league_replay_add(const drl_widenet_desc* d, int32_t members, const drl_replay* r, int64_t cursor,
                          int64_t num_envs, const void* d_codes_prev, const void* d_codes, const int32_t* d_actions,
                          const float* d_rewards, const uint8_t* d_dones, int32_t n_drones, hipStream_t stream) {
    drl::pop::Plan P;
    if (league_plan(d, members, 1, n_drones, &P)) return -1;
    if (const char* msg = drl::check_ring(r)) return fail(msg);
    if ((int64_t)r->obs_floats * 4 != drl::lay::code_bytes(P.P.code_w))
        return fail("a league's replay rows are policy codes (obs_floats = drl_policy_code_bytes / 4 words)");
    if ((uintptr_t)r->obs % 4 || (uintptr_t)r->next_obs % 4 || (uintptr_t)r->actions % 4 || (uintptr_t)r->rewards % 4)
        return fail("replay rows, actions and rewards must be 4-byte aligned");
    if (cursor < 0 || cursor >= r->capacity) return fail("cursor must be in [0, capacity)");
    if (num_envs < 1 || num_envs * n_drones >= ((int64_t)1 << 31))
        return fail("num_envs must be >= 1 (and num_envs * n_drones < 2^31)");
    if (check_codes(d_codes_prev, "the code rows (codes_prev)") || check_codes(d_codes, "the code rows (codes)")) return -1;
    if (!d_actions || !d_rewards || !d_dones || (uintptr_t)d_actions % 4 || (uintptr_t)d_rewards % 4)
        return fail("actions, rewards and dones must be non-NULL (actions and rewards 4-byte aligned)");
    drl::league::AddArgs a;
    memset(&a, 0, sizeof a);
    a.r_obs = reinterpret_cast<uint32_t*>(r->obs);
    a.r_next = reinterpret_cast<uint32_t*>(r->next_obs);
    a.r_act = r->actions;
    a.r_rew = r->rewards;
    a.r_done = r->dones;
    a.capacity = r->capacity;
    a.row_words = r->obs_floats;
    a.cursor = cursor;
    a.E = num_envs;
    a.total = num_envs * members;
    a.codes_prev = static_cast<const uint32_t*>(d_codes_prev);
    a.codes = static_cast<const uint32_t*>(d_codes);
    a.actions = d_actions;
    a.rewards = d_rewards;
    a.dones = d_dones;
    a.n_drones = n_drones;
    const int e = drl::league::launch_league_add(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_league_replay_add launch");
}

}  // extern "C"
