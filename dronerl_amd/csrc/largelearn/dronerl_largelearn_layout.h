// dronerl_largelearn_layout.h — the large-batch DQN learner's agent block (include/dronerl.h drl_dqn_large_*):
// the parameter sets' offsets (drl_dqn_layout_query's, so a block's sets read alike under both learners) and the
// scratch the launch chain hands from kernel to kernel: the sampled rows' decoded inputs, action, reward and done,
// every layer's activations of both nets, every layer's deltas, the rows' squared errors.  Plain C++ (no HIP):
// the host API, the kernels and tests/native/largelearn_layout_check.cpp share it.  The description itself is
// validated by dronerl_qnet_api.cpp's rule (the drl_qnet_desc limits); this header takes the layer sizes.
#ifndef DRONERL_LARGELEARN_LAYOUT_H
#define DRONERL_LARGELEARN_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"

#if defined(__HIPCC__)
#define DRL_LL_HD __host__ __device__ inline
#else
#define DRL_LL_HD inline
#endif

namespace drl {

struct DqnCounters;

namespace ll {

constexpr int kMaxLayers = 4;  // drl_qnet_desc: up to 3 hidden layers and the Q head (drl_dqn_layout's arrays)
constexpr int kMaxBatch = DRL_DQN_LARGE_MAX_BATCH;
constexpr int kMaxIn = 512, kMaxWidth = 128, kMaxActions = 8;  // drl_qnet_desc's limits
// the tile kernels (forward, backward): a workgroup of kTileThreads takes kTileRows sampled rows (one per lane)
// by kTileUnits outputs (kUnitsPerWave per wave), with the rows' operand staged in LDS kChunk columns at a time
constexpr int kTileRows = 64, kTileThreads = 256, kUnitsPerWave = 4;
constexpr int kTileUnits = kTileThreads / 64 * kUnitsPerWave;
constexpr int kChunk = 128, kChunkStride = kChunk + 4;  // (a row stride of 33 16-B slots: odd, so the lanes' reads spread)
// the update kernel: a workgroup takes kUpdateCols columns of [W_l | b_l] (the bias is column in[l]) by
// kUpdateUnits units, a thread one column of two units, with the rows staged in LDS kUpdateChunk at a time
constexpr int kUpdateThreads = 256, kUpdateCols = 64, kUpdateUnits = 8, kUpdateChunk = 64;
constexpr int kThreads = 256;                           // the element-wise kernels' workgroup

DRL_LL_HD int64_t r4(int64_t v) { return (v + 3) / 4 * 4; }

struct Plan {
    int32_t n_layers, batch, code_w;
    int32_t in4;                 // a decoded input row's stride: in[0] rounded up to 4 (the pad columns hold 0.0)
    int32_t in[kMaxLayers], out[kMaxLayers];
    int32_t ld[kMaxLayers];      // row stride of layer l's activations and deltas: out[l] rounded up to 4
    int64_t woff[kMaxLayers], boff[kMaxLayers], n_params;  // floats from a parameter set's start
    // words from the scratch's start; every region starts on a 16-byte boundary
    int64_t x_off[2];            // [batch][in4]: the rows' obs (0, the online net's input) and next_obs (1, the target's)
    int64_t act_off, rew_off, done_off;  // [batch]: int32 action, f32 reward, f32 done (0.0 / 1.0)
    int64_t h_off[2][kMaxLayers];  // [batch][ld[l]]: net n's relu(z_l) of a hidden layer, z of the Q head
    int64_t d_off[kMaxLayers];     // [batch][ld[l]]: dL/dz_l of the online net
    int64_t sq_off;                // [batch]: (q - td)^2
    int64_t scratch_words;
    drl_dqn_layout pub;
};

// Lay the agent block out for a dense net of n_layers layers (in[l] -> out[l]; a policy-code net: code_w = its
// window) and a batch.  max_width: the hidden widths' limit (drl_qnet_desc's by default; the wide nets' API,
// widenet/, passes its own: no kernel of the chain depends on it).  Returns nullptr, or the message for
// drl_last_error.
inline const char* plan(int n_layers, const int32_t* in, const int32_t* out, int code_w, int32_t batch, Plan* P,
                        int max_width = kMaxWidth) {
    if (!in || !out || !P) return "internal: the large-batch plan's arguments are NULL";
    if (batch < 1 || batch > kMaxBatch) return "batch must be in [1, 4096] (DRL_DQN_LARGE_MAX_BATCH)";
    if (n_layers < 2 || n_layers > kMaxLayers) return "n_hidden must be 1, 2 or 3";
    for (int l = 0; l < n_layers; ++l) {
        if (in[l] < 1 || in[l] > (l == 0 ? kMaxIn : max_width) || out[l] < 1 ||
            out[l] > (l + 1 < n_layers ? max_width : kMaxActions) || (l > 0 && in[l] != out[l - 1]))
            return "internal: layer sizes outside drl_qnet_desc's limits";
        if (l + 1 < n_layers && out[l] % 4) return "hidden widths must be multiples of 8 in [8, 128]";
    }
    *P = Plan{};
    P->n_layers = n_layers;
    P->batch = batch;
    P->code_w = code_w;
    P->in4 = (int32_t)r4(in[0]);
    drl_dqn_layout& o = P->pub;
    int64_t f = 0;  // (drl_dqn_layout_query's rule: each tensor padded to 4 floats)
    for (int l = 0; l < n_layers; ++l) {
        P->in[l] = in[l];
        P->out[l] = out[l];
        P->ld[l] = (int32_t)r4(out[l]);
        o.weight_off[l] = P->woff[l] = f;
        f += r4((int64_t)in[l] * out[l]);
        o.bias_off[l] = P->boff[l] = f;
        f += r4(out[l]);
    }
    o.n_params = P->n_params = f;
    const int64_t set = f * 4;
    o.online_off = 0;
    o.target_off = set;
    o.m_off = 2 * set;
    o.v_off = 3 * set;
    o.counters_off = 4 * set;
    o.scratch_off = o.counters_off + 64;  // sizeof(drl_dqn_counters)
    int64_t w = 0;
    auto take = [&w](int64_t words) {
        const int64_t at = w;
        w += r4(words);
        return at;
    };
    for (int n = 0; n < 2; ++n) P->x_off[n] = take((int64_t)batch * P->in4);
    P->act_off = take(batch);
    P->rew_off = take(batch);
    P->done_off = take(batch);
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < n_layers; ++l) P->h_off[n][l] = take((int64_t)batch * P->ld[l]);
    for (int l = 0; l < n_layers; ++l) P->d_off[l] = take((int64_t)batch * P->ld[l]);
    P->sq_off = take(batch);
    P->scratch_words = w;
    o.bytes = o.scratch_off + w * 4;
    o.grad_workgroups = 0;  // (no co-resident launch and no dynamic LDS: nothing to report)
    o.grad_lds_bytes = 0;
    return nullptr;
}

// ---- scratch words (from the scratch's start) of the chain's values ------------------------------------------
DRL_LL_HD int64_t x_word(const Plan& P, int net, int row, int k) { return P.x_off[net] + (int64_t)row * P.in4 + k; }
DRL_LL_HD int64_t h_word(const Plan& P, int net, int layer, int row, int j) {
    return P.h_off[net][layer] + (int64_t)row * P.ld[layer] + j;
}
DRL_LL_HD int64_t d_word(const Plan& P, int layer, int row, int j) {
    return P.d_off[layer] + (int64_t)row * P.ld[layer] + j;
}

// ---- the launches' grids ------------------------------------------------------------------------------------
DRL_LL_HD int row_tiles(const Plan& P) { return (P.batch + kTileRows - 1) / kTileRows; }
DRL_LL_HD int unit_tiles(int units) { return (units + kTileUnits - 1) / kTileUnits; }
// the update kernel's tiles of layer l, and the parameter (floats from a set's start) of unit j's column k:
// a weight for k < in[l], the bias for k == in[l]; -1 outside the layer
DRL_LL_HD int update_col_tiles(const Plan& P, int l) { return P.in[l] / kUpdateCols + 1; }
DRL_LL_HD int update_unit_tiles(const Plan& P, int l) { return (P.out[l] + kUpdateUnits - 1) / kUpdateUnits; }
DRL_LL_HD int64_t update_param(const Plan& P, int l, int j, int k) {
    if (j < 0 || j >= P.out[l] || k < 0 || k > P.in[l]) return -1;
    return k == P.in[l] ? P.boff[l] + j : P.woff[l] + (int64_t)j * P.in[l] + k;
}

// ---- kernel arguments (dronerl_largelearn.hip; launched by dronerl_largelearn_api.cpp) -----------------------
// (the field names dronerl_learn_common.h's functions read are the dense learner's)
struct LearnArgs {
    Plan P;
    int32_t trained;  // the host's plan: size >= batch (buffers.py can_sample)
    int32_t code_w;
    float* online;
    float* target;
    float* adam_m;
    float* adam_v;
    DqnCounters* ctr;
    float* scratch;
    uint32_t* pack_status;  // the act image's 16-B status vector (the counters kernel clears it before the pack)
    const uint32_t* r_obs;
    const uint32_t* r_next;
    int64_t row_words;  // words of a replay row
    const int32_t* r_act;
    const float* r_rew;
    const uint8_t* r_done;
    int64_t size;
    uint64_t seed;
    // hyperparameters, as the f32 constants jax's weak typing makes of the python floats
    float gamma, b1, b2, c1, c2, adam_eps, neg_lr, tau, one_minus_tau, eps_decay, eps_end;
    double b1d, b2d;
    int32_t target_every, eps_every;
};

// (hipError_t values) one learner step's launches in stream order, without the pack; the slots of the next step
int launch_large_train(const LearnArgs& a, hipStream_t s);
// ... and the segments of that chain which the prioritized chain (per/) launches as they are: every layer's
// forward; the backward pass and the update; the no-sample step's blend; the counters.  (No error is read: the
// caller reads hipGetLastError behind its last launch.)  The Double DQN chain (doubledqn/) takes the rows too.
void launch_large_rows(const LearnArgs& a, hipStream_t s);
void launch_large_forward(const LearnArgs& a, hipStream_t s);
void launch_large_backward_update(const LearnArgs& a, hipStream_t s);
void launch_large_blend(const LearnArgs& a, hipStream_t s);
void launch_large_counters(const LearnArgs& a, hipStream_t s);
int launch_large_sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s);

}  // namespace ll
}  // namespace drl
#endif
