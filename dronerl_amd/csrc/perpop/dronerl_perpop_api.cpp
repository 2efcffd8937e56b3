// dronerl_perpop_api.cpp — C ABI of the prioritized replay of a population of dense DQN agents (include/dronerl.h
// drl_pop_per_*; kernels in dronerl_perpop.hip, the layout in dronerl_perpop_layout.h).  Every call validates its
// arguments before any device work and names the offending one through drl_last_error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../../include/dronerl.h"
#include "../dronerl_host.h"
#include "../dronerl_internal.h"
#include "dronerl_perpop_layout.h"

using drl::fail;
using drl::hip_fail;

namespace {

using drl::perpop::ChainArgs;
using drl::perpop::TreeSetArgs;

// Every limit is checked here, by every call: nothing is refused at launch.
int pper_plan(int32_t members, int64_t capacity, int32_t max_batch, drl::perpop::Plan* P) {
    const char* msg = drl::perpop::plan(members, capacity, max_batch, P);
    return msg ? fail(msg) : 0;
}

int pper_block(int32_t members, int64_t capacity, int32_t max_batch, const void* d_pper, drl::perpop::Plan* P) {
    if (pper_plan(members, capacity, max_batch, P)) return -1;
    if (!d_pper || (uintptr_t)d_pper % 16)
        return fail("the prioritized population block must be a 16-byte aligned device pointer");
    return 0;
}

int pop_plan(const drl_widenet_desc* d, int32_t members, int32_t max_batch, drl::pop::Plan* P) {
    const char* msg = drl::pop::plan(d, members, max_batch, P);
    return msg ? fail(msg) : 0;
}

int pop_block(const void* d_pop) {
    if (!d_pop || (uintptr_t)d_pop % 16) return fail("the population block must be a 16-byte aligned device pointer");
    return 0;
}

void fill(TreeSetArgs* t, const drl::perpop::Plan& P, void* d_pper) {
    memset(t, 0, sizeof *t);
    t->T = P.T;
    t->members = P.members;
    t->stride = P.stride;
    t->hp_off = P.hp_off;
    t->base = static_cast<uint8_t*>(d_pper);
}

// the population's records and counters: the sampler's inputs and the gate of a train step
void fill_gate(TreeSetArgs* t, const drl::pop::Plan& Q, const void* d_pop, int64_t size) {
    t->gate = 1;
    t->pop = static_cast<const uint8_t*>(d_pop);
    t->pop_stride = Q.stride;
    t->pop_hp_off = Q.hp_off;
    t->pop_counters_off = Q.P.pub.counters_off;
    t->size = size;
}

}  // namespace

extern "C" {

int drl_pop_per_layout_query(int32_t members, int64_t capacity, int32_t max_batch, drl_pop_per_layout* layout) {
    drl::perpop::Plan P;
    if (pper_plan(members, capacity, max_batch, &P)) return -1;
    if (!layout) return fail("layout is NULL");
    memset(layout, 0, sizeof *layout);
    layout->member = P.T.pub;
    layout->member_stride = P.stride;
    layout->hparams_off = P.hp_off;
    layout->hparams_stride = drl::perpop::kPRecStride;
    layout->bytes = P.bytes;
    layout->members = members;
    layout->max_batch = max_batch;
    return 0;
}

int drl_pop_per_init(int32_t members, int64_t capacity, int32_t max_batch, const drl_per_hparams* ph, void* d_pper,
                     hipStream_t stream) {
    drl::perpop::Plan P;
    if (pper_plan(members, capacity, max_batch, &P)) return -1;
    if (!ph) return fail("the prioritized replay's hparams are NULL (a host array of `members` drl_per_hparams)");
    if (!d_pper || (uintptr_t)d_pper % 16)
        return fail("the prioritized population block must be a 16-byte aligned device pointer");
    char buf[160];
    for (int m = 0; m < members; ++m) {
        const char* what = nullptr;
        if (!(ph[m].alpha >= 0.0)) what = "alpha must be >= 0";
        else if (!(ph[m].beta0 >= 0.0 && ph[m].beta0 <= 1.0)) what = "beta0 must be in [0, 1]";
        else if (ph[m].beta_steps < 0) what = "beta_steps must be >= 0";
        else if (!(ph[m].eps >= 0.0)) what = "eps must be >= 0";
        if (what) {
            snprintf(buf, sizeof buf, "member %d: %s", m, what);
            return fail(buf);
        }
    }
    // the records, uploaded once: a train call takes no host hyperparameters
    std::vector<drl::perpop::PRec> recs((size_t)members);
    for (int m = 0; m < members; ++m) recs[m] = drl::perpop::PRec{ph[m].alpha, ph[m].beta0, ph[m].eps, ph[m].beta_steps};
    uint8_t* base = static_cast<uint8_t*>(d_pper);
    if (hipError_t e = hipMemcpyAsync(base + P.hp_off, recs.data(), recs.size() * sizeof recs[0], hipMemcpyHostToDevice,
                                      stream);
        e != hipSuccess)
        return hip_fail((int)e, "drl_pop_per_init records");
    if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess)  // (the host table is gone after the call)
        return hip_fail((int)e, "drl_pop_per_init records");
    TreeSetArgs t;
    fill(&t, P, d_pper);
    const int e = drl::perpop::launch_init(t, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_pop_per_init launch");
}

int drl_pop_per_mark_new(int32_t members, int64_t capacity, int32_t max_batch, void* d_pper, int64_t cursor,
                         int64_t count, hipStream_t stream) {
    drl::perpop::Plan P;
    if (pper_block(members, capacity, max_batch, d_pper, &P)) return -1;
    if (cursor < 0 || cursor >= capacity) return fail("cursor must be in [0, capacity)");
    if (count < 0) return fail("count must be >= 0");
    TreeSetArgs t;
    fill(&t, P, d_pper);
    const int e = drl::perpop::launch_mark(t, cursor, count, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_pop_per_mark_new launch");
}

int drl_pop_per_rebuild(int32_t members, int64_t capacity, int32_t max_batch, void* d_pper, hipStream_t stream) {
    drl::perpop::Plan P;
    if (pper_block(members, capacity, max_batch, d_pper, &P)) return -1;
    TreeSetArgs t;
    fill(&t, P, d_pper);
    const int e = drl::perpop::launch_rebuild(t, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_pop_per_rebuild launch");
}

int drl_pop_per_sample(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop, void* d_pper,
                       int64_t capacity, int64_t size, hipStream_t stream) {
    drl::pop::Plan Q;
    drl::perpop::Plan P;
    if (pop_plan(d, members, max_batch, &Q)) return -1;
    if (pop_block(d_pop)) return -1;
    if (pper_block(members, capacity, max_batch, d_pper, &P)) return -1;
    if (size < 1 || size > capacity) return fail("size must be in [1, capacity] (nothing is drawn from an empty ring)");
    TreeSetArgs t;
    fill(&t, P, d_pper);
    fill_gate(&t, Q, d_pop, size);
    const int e = drl::perpop::launch_sample(t, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_pop_per_sample launch");
}

int drl_pop_per_train(const drl_widenet_desc* d, int32_t members, int32_t max_batch, void* d_pop, const drl_replay* r,
                      int64_t size, void* d_pper, hipStream_t stream) {
    drl::pop::Plan Q;
    drl::perpop::Plan P;
    if (pop_plan(d, members, max_batch, &Q)) return -1;
    if (pop_block(d_pop)) return -1;
    if (!r || !r->obs || !r->next_obs || !r->actions || !r->rewards || !r->dones) return fail("replay buffers are NULL");
    if ((int64_t)r->obs_floats * 4 != drl::lay::code_bytes(Q.P.code_w))
        return fail("a population's replay rows are policy codes (obs_floats = drl_policy_code_bytes / 4 words)");
    if ((uintptr_t)r->obs % 4 || (uintptr_t)r->next_obs % 4 || (uintptr_t)r->actions % 4 || (uintptr_t)r->rewards % 4)
        return fail("replay rows, actions and rewards must be 4-byte aligned");
    if (pper_block(members, r->capacity, max_batch, d_pper, &P)) return -1;
    if (size < 0 || size > r->capacity) return fail("size must be in [0, capacity]");
    ChainArgs a;
    memset(&a, 0, sizeof a);
    a.p.P = Q.P;
    a.p.members = Q.members;
    a.p.n_actions = Q.n_actions;
    a.p.stride = Q.stride;
    a.p.hp_off = Q.hp_off;
    a.p.base = static_cast<uint8_t*>(d_pop);
    a.p.r_obs = reinterpret_cast<uint32_t*>(r->obs);
    a.p.r_next = reinterpret_cast<uint32_t*>(r->next_obs);
    a.p.r_act = r->actions;
    a.p.r_rew = r->rewards;
    a.p.r_done = r->dones;
    a.p.capacity = r->capacity;
    a.p.row_words = r->obs_floats;
    a.p.size = size;
    fill(&a.t, P, d_pper);
    fill_gate(&a.t, Q, d_pop, size);
    const int e = drl::perpop::launch_train(a, stream);
    return e == 0 ? 0 : hip_fail(e, "drl_pop_per_train launch");
}

}  // extern "C"
