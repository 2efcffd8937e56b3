// dronerl_convpop_api.cpp — C ABI of the population of conv DQN agents (include/dronerl.h drl_convpop_*; kernels
// in dronerl_convpop.hip, the layout in dronerl_convpop_layout.h).  Every call validates its arguments before any
// device work and names the offending field through drl_last_error.  The rings are the dense population's
// (drl_pop_replay_add).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "../dronerl_internal.h"
#include "../dronerl_learn_args.h"
#include "dronerl_convpop_layout.h"

using drl::fail;
using drl::hip_fail;

namespace {

// Every limit is checked here, by every call: nothing is refused at launch.
int cp_plan(const drl_convnet_desc* d, int32_t members, int32_t max_batch, drl::cp::Plan* P) {
    const char* msg = drl::cp::plan(d, members, max_batch, P);
    return msg ? fail(msg) : 0;
}

int check_block(const void* d_pop) {
    if (!d_pop || (uintptr_t)d_pop % 16) return fail("the population block must be a 16-byte aligned device pointer");
    return 0;
}

// the rings of a population: drl_replay's arrays, [members][capacity] each
int check_rings(const drl::cp::Plan& P, const drl_replay* r) {
    if (const char* msg = drl::check_ring(r)) return fail(msg);
    if ((int64_t)r->obs_floats * 4 != drl::lay::code_bytes(P.code_w))
        return fail("a population's replay rows are policy codes (obs_floats = drl_policy_code_bytes / 4 words)");
    if ((uintptr_t)r->obs % 4 || (uintptr_t)r->next_obs % 4 || (uintptr_t)r->actions % 4 || (uintptr_t)r->rewards % 4)
        return fail("replay rows, actions and rewards must be 4-byte aligned");
    return 0;
}

void fill(drl::cp::PopArgs* a, const drl::cp::Plan& P, void* d_pop) {
    memset(a, 0, sizeof *a);
    a->P = P.P.c;
    a->t = P.P.t;
    a->members = P.members;
    a->stride = P.stride;
    a->hp_off = P.hp_off;
    a->base = static_cast<uint8_t*>(d_pop);
}

}  // namespace

extern "C" {

int drl_convpop_layout_query(const drl_convnet_desc* d, int32_t members, int32_t max_batch, drl_convpop_layout* layout) {
    drl::cp::Plan P;
    if (cp_plan(d, members, max_batch, &P)) return -1;
    if (!layout) return fail("layout is NULL");
    memset(layout, 0, sizeof *layout);
    layout->member = P.P.c.pub;
    layout->member_stride = P.stride;
    layout->hparams_off = P.hp_off;
    layout->hparams_stride = drl::cp::kHRecStride;
    layout->bytes = P.bytes;
    layout->members = members;
    layout->max_batch = max_batch;
    return 0;
}

int drl_convpop_init(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const drl_dqn_hparams* h,
                     const float* epsilon_start, void* d_pop, hipStream_t stream) {
    drl::cp::Plan P;
    if (cp_plan(d, members, max_batch, &P)) return -1;
    if (!h) return fail("hparams is NULL (a host array of `members` drl_dqn_hparams)");
    if (!epsilon_start) return fail("epsilon_start is NULL (a host array of `members` floats)");
    if (check_block(d_pop)) return -1;
    char buf[160];
    for (int m = 0; m < members; ++m) {
        const char* what = nullptr;
        if (h[m].batch < 1 || h[m].batch > max_batch) what = "batch must be in [1, max_batch]";
        else what = drl::check_hparam_ranges(&h[m]);
        if (what) {
            snprintf(buf, sizeof buf, "member %d: %s", m, what);
            return fail(buf);
        }
    }
    // the records, uploaded once: a train call takes no host hyperparameters
    std::vector<uint8_t> recs((size_t)(drl::cp::kHRecStride * members), 0);
    for (int m = 0; m < members; ++m) {
        drl::cp::HRec r = drl::pop::hrec_of(h[m]);
        r.eps_start = epsilon_start[m];
        memcpy(recs.data() + drl::cp::kHRecStride * m, &r, sizeof r);
    }
    uint8_t* base = static_cast<uint8_t*>(d_pop);
    if (hipError_t e = hipMemcpyAsync(base + P.hp_off, recs.data(), recs.size(), hipMemcpyHostToDevice, stream);
        e != hipSuccess)
        return hip_fail((int)e, "drl_convpop_init records");
    if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess)  // (the host table is gone after the call)
        return hip_fail((int)e, "drl_convpop_init records");
    drl::cp::PopArgs a;
    fill(&a, P, d_pop);
    const int e = drl::cp::launch_convpop_init(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convpop_init launch");
}

int drl_convpop_act(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop, const void* d_code,
                    int64_t envs_per_member, int32_t greedy, uint64_t seed, uint64_t step, int64_t env_offset,
                    int32_t* d_actions, int32_t n_drones, uint64_t synth_seed, uint64_t synth_step, float* d_q,
                    hipStream_t stream) {
    drl::cp::Plan P;
    if (cp_plan(d, members, max_batch, &P)) return -1;
    if (check_block(d_pop)) return -1;
    if (!d_code || (uintptr_t)d_code % 16) return fail("the policy code must be a 16-byte aligned device pointer");
    if (envs_per_member < 1 || envs_per_member * members >= ((int64_t)1 << 31))
        return fail("envs_per_member must be >= 1 (and members * envs_per_member < 2^31)");
    if (!d_actions || (uintptr_t)d_actions % 4 || (uintptr_t)d_q % 4) return fail("actions must be non-NULL; actions and q 4-byte aligned");
    if (n_drones < 1 || n_drones > DRL_MAX_DRONES) return fail("n_drones must be in [1, 64]");
    drl::cp::ActArgs a;
    memset(&a, 0, sizeof a);
    a.P = P.P.c;
    a.members = members;
    a.stride = P.stride;
    a.base = static_cast<const uint8_t*>(d_pop);
    a.code = static_cast<const uint32_t*>(d_code);
    a.row_words = drl::lay::code_bytes(P.code_w) / 4;
    a.E = envs_per_member;
    a.greedy = greedy ? 1 : 0;
    a.seed = seed;
    a.step = step;
    a.env_offset = env_offset;
    a.actions = d_actions;
    a.n_drones = n_drones;
    a.synth_seed = synth_seed;
    a.synth_step = synth_step;
    a.q = d_q;
    // (the rows kernel's workgroup: a row's arithmetic does not depend on the thread count)
    const int e = drl::cp::launch_convpop_act(a, P.P.t.rows_threads, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convpop_act launch");
}

int drl_convpop_train(const drl_convnet_desc* d, int32_t members, int32_t max_batch, void* d_pop, const drl_replay* r,
                      int64_t size, hipStream_t stream) {
    drl::cp::Plan P;
    if (cp_plan(d, members, max_batch, &P)) return -1;
    if (check_block(d_pop)) return -1;
    if (check_rings(P, r)) return -1;
    if (size < 0 || size > r->capacity) return fail("size must be in [0, capacity]");
    drl::cp::PopArgs a;
    fill(&a, P, d_pop);
    a.r_obs = reinterpret_cast<const uint32_t*>(r->obs);
    a.r_next = reinterpret_cast<const uint32_t*>(r->next_obs);
    a.r_act = r->actions;
    a.r_rew = r->rewards;
    a.r_done = r->dones;
    a.capacity = r->capacity;
    a.row_words = r->obs_floats;
    a.size = size;
    const int e = drl::cp::launch_convpop_train(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convpop_train launch");
}

int drl_convpop_sample_rows(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                            int64_t size, int64_t* d_slots, hipStream_t stream) {
    drl::cp::Plan P;
    if (cp_plan(d, members, max_batch, &P)) return -1;
    if (check_block(d_pop)) return -1;
    if (!d_slots || (uintptr_t)d_slots % 8) return fail("d_slots must be an 8-byte aligned device pointer");
    if (size < 1) return fail("size must be >= 1 (buffers.py can_sample: nothing is drawn from an empty ring)");
    drl::cp::PopArgs a;
    fill(&a, P, const_cast<void*>(d_pop));
    a.size = size;
    a.slots = d_slots;
    const int e = drl::cp::launch_convpop_sample(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_convpop_sample_rows launch");
}

}  // extern "C"
