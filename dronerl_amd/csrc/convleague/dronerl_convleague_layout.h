// dronerl_convleague_layout.h — a league of conv learners: K members of a drl_convpop_layout block acting in the
// SAME E envs, learner k on drone index k (include/dronerl.h drl_convleague_*).  The block, the records, the rings
// and the learner chain are the conv population's (convpop/dronerl_convpop_layout.h) and the add is the league's
// (league/dronerl_league_layout.h), all unchanged; this header adds the act's plan and its kernel's arguments.
// Plain C++ (no HIP): the host API, the kernel and tests/native/convleague_layout_check.cpp share it.
//
// The act's tiling (few members, thousands of envs each).  A workgroup takes env_tile = T envs of one member
// through every layer, so a weight word fetched from L2 serves T envs: a conv layer's thread owns one output
// element of all T envs (the tap's weight loaded once, T accumulators in registers), a dense layer's wave owns one
// unit of all T envs (lane c loads w[c], w[c + 64], .. once and keeps T partial sums).  Each env has one compact
// forward-only row in LDS: the input x at word 0, then every layer's output (relu(z); the head: z), each rounded
// up to 4 words.  The dL/dz words cl::Plan reserves for the backward are left out, so a row never is larger than
// cl::Plan::row_words (at most 64 KB) and T = 2 fits every net cg::plan accepts.  T is the largest of kEnvTiles
// whose rows fit kLdsLimit.
#ifndef DRONERL_CONVLEAGUE_LAYOUT_H
#define DRONERL_CONVLEAGUE_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../convpop/dronerl_convpop_layout.h"

namespace drl {
namespace cvl {

constexpr int kEnvTiles[] = {16, 8, 4, 2};  // the choices of T, largest first
constexpr int kNumEnvTiles = 4;
constexpr int kMaxEnvTile = 16;
constexpr int kLdsLimit = 160 * 1024;  // a CU's LDS (MI355X), as league::kLdsLimit
// the workgroup: a multiple of 256 threads by the widest layer, up to kThreadsMax (a row's arithmetic does not
// depend on the count: a conv element is one thread's, a dense unit one wave's)
constexpr int kThreadsMin = 256, kThreadsMax = 1024;

struct ActPlan {
    int32_t env_tile, threads;
    int32_t row_words;              // the row stride (words): the compact row, a multiple of 4
    int32_t lds_bytes;              // env_tile * row_words * 4
    int32_t out[cl::kMaxLayers];    // words from a row's start: layer l's output (layer l + 1's input)
    int32_t n_layers;
};

// words from a row's start of layer l's input: x at word 0, else the previous layer's output
DRL_CV_HD int in_word(const ActPlan& A, int l) { return l == 0 ? 0 : A.out[l - 1]; }
// LDS word of word w of env r's row
DRL_CV_HD int lds_word(const ActPlan& A, int r, int w) { return r * A.row_words + w; }

// The compact row of a validated learner plan (every T shares it).
inline int32_t compact_row(const cl::Plan& P, int32_t* out) {
    int64_t word = cl::r4(P.in);
    for (int l = 0; l < P.n_layers; ++l) {
        out[l] = (int32_t)word;
        word = cl::r4(word + P.l[l].n_out);
    }
    return (int32_t)word;
}

// The plan with the env tile forced to T (the checker calls it with every T; act_plan with the list).
inline const char* act_plan_for(const cl::Plan& P, int T, ActPlan* out) {
    if (!out) return "internal: the conv league act plan is NULL";
    *out = ActPlan{};
    out->n_layers = P.n_layers;
    out->row_words = compact_row(P, out->out);
    if (out->row_words > P.row_words) return "internal: the forward-only row exceeds the learner's row";
    int widest = 0;
    for (int l = 0; l < P.n_layers; ++l) widest = P.l[l].n_out > widest ? P.l[l].n_out : widest;
    int t = (widest + kThreadsMin - 1) / kThreadsMin * kThreadsMin;
    out->threads = t < kThreadsMin ? kThreadsMin : t > kThreadsMax ? kThreadsMax : t;
    out->env_tile = T;
    const int64_t bytes = (int64_t)T * out->row_words * 4;
    if (bytes > kLdsLimit) return "internal: the conv league act's LDS plan exceeds a CU's 160 KiB";
    out->lds_bytes = (int32_t)bytes;
    return nullptr;
}

// The act's plan for a validated population plan: the largest T of kEnvTiles that fits.  Returns nullptr, or the
// message for drl_last_error.
inline const char* act_plan(const cp::Plan& p, ActPlan* out) {
    const char* msg = "internal: the conv league act plan has no env tile";
    for (int i = 0; i < kNumEnvTiles; ++i)
        if (!(msg = act_plan_for(p.P.c, kEnvTiles[i], out))) return nullptr;
    return msg;
}

// ---- kernel arguments (dronerl_convleague.hip; launched by dronerl_convleague_api.cpp) -----------------------
struct ActArgs {
    cl::Plan P;
    ActPlan A;
    int32_t members;
    int64_t stride;          // bytes from one member block to the next
    const uint8_t* base;
    const uint32_t* codes;   // [n_drones][E][row_words]: drl_obs_code_all's output (learner k reads block k)
    int64_t row_words, E;    // words of a code row; envs
    int32_t greedy, n_drones;
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;        // [E][n_drones]: columns 0 .. members - 1 are written
    float* q;                // nullable: [members][E][n_actions]
};

// (a hipError_t value)
int launch_convleague_act(const ActArgs& a, hipStream_t s);

}  // namespace cvl
}  // namespace drl
#endif
