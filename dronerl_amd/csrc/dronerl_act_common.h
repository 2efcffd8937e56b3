// dronerl_act_common.h — the contract code every act kernel shares (device only: included by the .hip units,
// never by the .cpp files): the two counter-hash action streams, the epsilon-greedy epilogue, the range flag and
// the up-front LDS staging of a packed image.  The streams are bit-exact contracts between the dense and conv
// acts, the step, drl_synth_actions, the oracle and the tests' _hash_explore: each has its one definition here.
// The functions take scalars or an args struct as a template argument (drl::QnetArgs, drl::cv::ActArgs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dronerl.h"

namespace drl {

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// The synthetic action stream (drl_synth_actions, the oracle's synth_actions): drone `drone` of global env
// `genv` at (seed, step) -- a counter hash, so any kernel can draw any element.
__device__ __forceinline__ int synth_action(uint64_t seed, uint64_t step, uint64_t genv, uint64_t drone) {
    const uint64_t h = splitmix64(seed ^ splitmix64((step << 40) ^ (genv << 8) ^ drone));
    return (int)(((h >> 32) * 5ull) >> 32);
}

// The exploration stream of drone 0 (DQNAgent.act: uniform < epsilon ? random action : argmax Q): the random
// action when global env `genv` explores at (seed, step), else -1.  Independent of Q.
__device__ __forceinline__ int explore_draw(uint64_t seed, uint64_t step, uint64_t genv, int n_actions, float eps) {
    const uint64_t hsh = splitmix64(seed ^ splitmix64((step << 40) ^ (genv << 8) ^ 0xa5ull));
    const float u = (float)(hsh >> 40) * (1.0f / 16777216.0f);
    const int rnd = (int)(((hsh & 0xffffffffull) * (uint64_t)n_actions) >> 32);
    return u < eps ? rnd : -1;
}

// The exploration rate: the argument, or a learner's device counter (drl_qnet_act_eps).
template <class Args>
__device__ __forceinline__ float act_eps(const Args& a) {
    return a.eps_ptr ? *a.eps_ptr : a.epsilon;
}

// jnp.argmax over q[0 .. n_actions): the first maximum (selects, no register-array index).
__device__ __forceinline__ int argmax_first(const float (&q)[8], int n_actions) {
    int best = 0;
    float qb = q[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const bool b = i < n_actions && q[i] > qb;
        best = b ? i : best;
        qb = b ? q[i] : qb;
    }
    return best;
}

// Drone 0's action of env `env` (explore: explore_draw's value; best: the argmax), and its Q row where the
// caller asked for one.
template <class Args>
__device__ __forceinline__ void store_act(const Args& a, int64_t env, int explore, int best) {
    a.actions[env * a.action_stride] = explore >= 0 ? explore : best;
}
template <class Args>
__device__ __forceinline__ void store_q(const Args& a, int64_t env, const float (&q)[8], int n_actions) {
    if (a.q) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < n_actions) a.q[env * n_actions + i] = q[i];
    }
}

// The whole epilogue of one env whose Q row is in registers.
template <class Args>
__device__ __forceinline__ void act_epilogue(const Args& a, int64_t env, const float (&q)[8], int n_actions,
                                             bool with_q = true) {
    const int explore = explore_draw(a.seed, a.step, (uint64_t)(a.env_offset + env), n_actions, act_eps(a));
    store_act(a, env, explore, argmax_first(q, n_actions));
    if (with_q) store_q(a, env, q, n_actions);
}

// The epilogue of a 16-env output tile whose accumulator holds Q (column = env): own(i), i = 0..3, is the lane's
// register i with the bias added -- actions 0..3 in the g = 0 lane of env column c, 4..7 in its g = 1 lane, which
// the g = 0 lane fetches and then acts for env `env` (every lane calls; lanes of envs >= E store nothing).
template <class Args, class F>
__device__ __forceinline__ void tile_act(const Args& a, int64_t env, int lane, F own, bool with_q = true) {
    float q[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        q[i] = own(i);
        q[i + 4] = __shfl(q[i], (lane & 15) + 16);
    }
    if ((lane >> 4) == 0 && env < a.E) act_epilogue(a, env, q, a.n_actions, with_q);
}

// drl_synth_actions' columns 1..synth_n-1 of this wave's envs (groups grp0, grp0 + gstride, .. < gend of EPG
// envs each), after the act: stores issued before the net's LDS-DMA wait (vmcnt counts them) would delay the
// first group.
template <int EPG, class Args>
__device__ __forceinline__ void synth_tail(const Args& a, int64_t grp0, int64_t gend, int64_t gstride, int lane) {
    if (a.synth_n <= 1) return;
    const uint32_t nd = (uint32_t)a.synth_n - 1u;
    const uint32_t per = (uint32_t)EPG * nd;
    for (int64_t gg = grp0; gg < gend; gg += gstride) {
        for (uint32_t k = (uint32_t)lane; k < per; k += 64u) {
            const uint32_t el = k / nd;
            const int64_t env = EPG * gg + el;
            const uint64_t drone = 1u + (k - el * nd);
            if (env < a.E)
                a.actions[env * a.action_stride + (int64_t)drone] =
                    synth_action(a.synth_seed, a.synth_step, (uint64_t)(a.env_offset + env), drone);
        }
    }
}

// DRL_ERR_QNET_RANGE when a lane of the wave saw an operand outside fp16's range (`bad`) or the pack did (its
// status word).
__device__ __forceinline__ void flag_qnet_range(int32_t* err, const void* pack_status, bool bad, int lane) {
    bad |= lane == 0 && *static_cast<const int32_t*>(pack_status) != 0;
    if (__ballot(bad) && lane == 0 && err) atomicOr(err, DRL_ERR_QNET_RANGE);
}

// The packed image's first lds_vec 16-B vectors into LDS by LDS-DMA (no registers; every piece in flight at
// once), then the wait for this wave's and the barrier for every wave's.
__device__ __forceinline__ void stage_packed_lds(uint4* wl, const uint4* packed, int lds_vec, int wave, int nwaves,
                                                 int lane) {
    for (int v0 = wave * 64; v0 < lds_vec; v0 += 64 * nwaves)
        if (v0 + lane < lds_vec)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(packed + v0 + lane),
                                             (__attribute__((address_space(3))) void*)(wl + v0), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

}  // namespace drl
