// dronerl_convlearn_layout.h — the conv DQN learner's agent block (include/dronerl.h drl_convnet_dqn_*): the
// parameter sets' offsets, the parameter index <-> (layer, co, ci, ky, kx) map of the update kernel, and the
// per-row scratch (inputs, activations, deltas) the rows kernel hands to it.  Plain C++ (no HIP): the host API,
// the kernels and tests/native/convlearn_layout_check.cpp share it.  The net's shape arithmetic is
// convnet/dronerl_convnet_layout.h's.
#ifndef DRONERL_CONVLEARN_LAYOUT_H
#define DRONERL_CONVLEARN_LAYOUT_H

#include <stdint.h>

#include "../convnet/dronerl_convnet_layout.h"

namespace drl {

struct DqnCounters;

namespace cl {

constexpr int kMaxLayers = cv::kMaxLayers;  // 3 conv + 2 hidden dense + the Q head
static_assert(kMaxLayers == DRL_CONVNET_DQN_MAX_LAYERS, "drl_convnet_dqn_layout's arrays");
constexpr int kMaxBatch = 64;
constexpr int kRowsThreads = 256;    // the rows kernel's workgroup (one per sampled row)
constexpr int kUpdateThreads = 256;  // the update kernel's workgroup (a thread per dense parameter, a wave per conv one)
// the rows kernel keeps one row's input, activations and deltas in LDS: at most this many bytes
constexpr int kRowLdsMax = DRL_CONVNET_DQN_ROW_BYTES_MAX;

// One layer as the learner sees it.  Activations and deltas are in torch order: conv [co][oy][ox] (so the
// flatten is the identity and the first dense layer's columns index it directly), dense [unit].
struct LLayer {
    int32_t conv, cin, cout, k, s, p, in_side, out_side;
    int32_t n_in, n_out;   // elements of the layer's input / output per row
    int32_t K;             // weights per output (conv: cin * k * k; dense: n_in)
    int32_t in;            // words from a row's start: the layer's input (the row's x, or the previous act)
    int32_t act;           // words from a row's start: relu(z) (-1: the Q head keeps none)
    int32_t delta;         // words from a row's start: dL/dz
    int64_t woff, boff;    // floats from a parameter set's start
};

struct Plan {
    int32_t n_conv, n_layers, window, code_w, n_actions, batch;
    int32_t in;         // W * W * 6: the row's input x, [y][x][c] as the observation has it, at word 0 of the row
    int32_t row_words;  // scratch words per sampled row (a multiple of 4)
    int64_t sq_off, rows_off, scratch_words;  // words from the scratch's start: squared errors [64], rows [batch]
    int64_t n_params;
    LLayer l[kMaxLayers];
    drl_convnet_dqn_layout pub;
};

inline int64_t r4(int64_t v) { return (v + 3) / 4 * 4; }

// Validate a description and a batch and lay the agent block out.  Returns nullptr, or the message for
// drl_last_error.
inline const char* plan(const drl_convnet_desc* d, int32_t batch, Plan* P) {
    cv::Layout L;
    if (const char* msg = cv::layout(d, &L)) return msg;
    if (batch < 1 || batch > kMaxBatch) return "batch must be in [1, 64]";
    *P = Plan{};
    P->n_conv = L.n_conv;
    P->n_layers = L.n_layers;
    P->window = L.window;
    P->code_w = L.input == DRL_QNET_INPUT_CODE ? L.window : 0;
    P->n_actions = L.n_actions;
    P->batch = batch;
    P->in = L.window * L.window * 6;
    int64_t par = 0, word = r4(P->in);
    for (int i = 0; i < L.n_layers; ++i) {
        const cv::Layer& y = L.l[i];
        LLayer& q = P->l[i];
        q.conv = y.conv;
        if (y.conv) {
            q.cin = y.cin;
            q.cout = y.cout;
            q.k = y.k;
            q.s = y.s;
            q.p = y.p;
            q.in_side = y.in_side;
            q.out_side = y.out_side;
            q.n_in = y.cin * y.in_side * y.in_side;
            q.n_out = y.cout * y.out_side * y.out_side;
        } else {
            q.cin = y.K;
            q.cout = y.N;
            q.k = q.s = 1;
            q.in_side = q.out_side = 1;
            q.n_in = y.K;
            q.n_out = y.N;
        }
        q.K = y.K;
        q.woff = par;
        par += (int64_t)q.cout * q.K;
        q.boff = par;
        par += q.cout;
        q.in = i == 0 ? 0 : P->l[i - 1].act;
        q.act = -1;
        if (i + 1 < L.n_layers) {
            q.act = (int32_t)word;
            word = r4(word + q.n_out);
        }
        q.delta = (int32_t)word;
        word = r4(word + q.n_out);
    }
    if (word * 4 > kRowLdsMax)
        return "the conv learner's per-row working set (input, activations and deltas of every layer) exceeds "
               "DRL_CONVNET_DQN_ROW_BYTES_MAX (64 KB of LDS): window, padding and out_channels";
    P->row_words = (int32_t)word;
    P->n_params = par;
    P->sq_off = 0;
    P->rows_off = kMaxBatch;
    P->scratch_words = P->rows_off + (int64_t)batch * P->row_words;
    drl_convnet_dqn_layout& u = P->pub;
    u.n_params = par;
    u.n_layers = L.n_layers;
    for (int i = 0; i < L.n_layers; ++i) {
        u.weight_off[i] = P->l[i].woff;
        u.bias_off[i] = P->l[i].boff;
    }
    const int64_t set = (par * 4 + 15) / 16 * 16;
    u.online_off = 0;
    u.target_off = set;
    u.m_off = 2 * set;
    u.v_off = 3 * set;
    u.counters_off = 4 * set;
    u.scratch_off = u.counters_off + 64;
    u.bytes = u.scratch_off + P->scratch_words * 4;
    u.row_bytes = P->row_words * 4;
    return nullptr;
}

// ---- the parameter index <-> tensor element map (the update kernel: one thread per parameter) ---------------
// conv weight [co][ci][ky][kx], dense weight [co = out][ci = in] (ky = kx = 0), bias [co] (torch layouts)
struct ParamRef {
    int32_t layer, bias, co, ci, ky, kx;
};

DRL_CV_HD int64_t param_index(const Plan& P, const ParamRef& r) {
    const LLayer& q = P.l[r.layer];
    if (r.bias) return q.boff + r.co;
    return q.woff + (((int64_t)r.co * q.cin + r.ci) * q.k + r.ky) * q.k + r.kx;
}

DRL_CV_HD ParamRef param_locate(const Plan& P, int64_t i) {
    int l = 0;
    while (l + 1 < P.n_layers && i >= P.l[l + 1].woff) ++l;
    const LLayer& q = P.l[l];
    ParamRef r{l, 0, 0, 0, 0, 0};
    if (i >= q.boff) {
        r.bias = 1;
        r.co = (int32_t)(i - q.boff);
        return r;
    }
    int32_t e = (int32_t)(i - q.woff);
    r.co = e / q.K;
    e -= r.co * q.K;
    const int kk = q.k * q.k;
    r.ci = e / kk;
    e -= r.ci * kk;
    r.ky = e / q.k;
    r.kx = e - r.ky * q.k;
    return r;
}

// word (from the scratch's start) of element e of a row's input (layer < 0), of layer's activation (which = 0)
// or delta (which = 1)
DRL_CV_HD int64_t row_word(const Plan& P, int row, int layer, int which, int e) {
    const int64_t base = P.rows_off + (int64_t)row * P.row_words;
    if (layer < 0) return base + e;
    return base + (which ? P.l[layer].delta : P.l[layer].act) + e;
}

// ---- kernel arguments (dronerl_convlearn.hip; launched by dronerl_convlearn_api.cpp) ------------------------
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

// (hipError_t values) the rows, update and counters launches of one learner step, in stream order
int launch_convnet_dqn_train(const LearnArgs& a, hipStream_t s);

}  // namespace cl
}  // namespace drl
#endif
