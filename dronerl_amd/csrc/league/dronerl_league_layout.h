// dronerl_league_layout.h — a league: K learners ("members" of a drl_pop_layout block) acting in the SAME E envs,
// learner k on drone index k (include/dronerl.h drl_league_*).  The block, the records and the rings are the
// population's (population/dronerl_population_layout.h), unchanged; this header adds the act's plan and the two
// kernels' arguments.  Plain C++ (no HIP): the host API, the kernels and tests/native/league_layout_check.cpp
// share it.
//
// The act's tiling (few members, thousands of envs each).  A workgroup of kActThreads takes kEnvTile envs of one
// member through every layer.  A wave's lanes are kEnvTile envs x 2 unit halves; a lane holds kUnitsPerLane
// units of its env in registers (the four partial sums of each), so a pass of the workgroup computes
// kPassUnits = waves x 2 x kUnitsPerLane units of the kEnvTile envs.  The weights of a pass come kChunkK columns
// at a time: read once from the member's online set, coalesced, staged in LDS as [kPassUnits][kChunkK] (pad
// columns and units hold 0.0), and read back at half-wave-uniform addresses (a broadcast), so one weight read
// serves 32 envs.  The envs' rows (the decoded inputs, then the layers' activations) live in two LDS regions that
// alternate: layer l reads region l & 1 and writes the other.  A row stride is a multiple of 4 floats whose
// quarter is odd, so the 16 lanes a ds_read_b128 serves together (16 different envs) fall on 16 different
// 16-byte bank groups.
#ifndef DRONERL_LEAGUE_LAYOUT_H
#define DRONERL_LEAGUE_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../population/dronerl_population_layout.h"

namespace drl {
namespace league {

constexpr int kActThreads = 256, kEnvTile = 32, kUnitsPerLane = 8;
constexpr int kPassUnits = kActThreads / 64 * 2 * kUnitsPerLane;  // 64
constexpr int kChunkK = 32;
constexpr int kStageLoads = kPassUnits * kChunkK / kActThreads;  // staged floats per thread and chunk
constexpr int kLdsLimit = 160 * 1024;                            // a CU's LDS (MI355X): a workgroup may use all of it
constexpr int kThreads = 256;                                    // the add kernel's workgroup
static_assert(kEnvTile == 32 && kActThreads % 64 == 0, "a wave is 32 envs x 2 unit halves");
static_assert(kChunkK % 4 == 0 && kUnitsPerLane % 4 == 0, "16-byte LDS reads and stores");
static_assert(kPassUnits * kChunkK % kActThreads == 0 && kActThreads % kChunkK == 0, "the staging map");

struct ActPlan {
    int32_t ldx, lda;            // row strides (floats): the decoded inputs; a layer's activations
    int32_t a_floats, b_floats;  // the two row regions: layer l reads region l & 1 (A first) and writes the other
    int32_t w_floats;            // the staged weight chunk
    int32_t lds_bytes;
};

DRL_LL_HD int r8(int v) { return (v + 7) / 8 * 8; }
// the smallest stride >= v that is a multiple of 4 with an odd quarter
DRL_LL_HD int odd_quarter(int v) {
    const int s = (v + 3) / 4 * 4;
    return (s / 4) % 2 ? s : s + 4;
}
// passes over a layer's J units, chunks over its K inputs, 4-column steps of chunk c (the last may be short; the
// columns K .. r4(K) - 1 it covers hold 0.0 on both sides).  The count is even for every accepted net (hidden
// widths are multiples of 8, W * W * 6 rounded up to 4 is a multiple of 8 for W = 5, 7, 9): the kernel takes two
// steps per turn, and act_plan refuses a net for which it is not.
DRL_LL_HD int pass_count(int J) { return (J + kPassUnits - 1) / kPassUnits; }
DRL_LL_HD int chunk_count(int K) { return (K + kChunkK - 1) / kChunkK; }
DRL_LL_HD int chunk_quads(int K, int c) {
    const int left = (K + 3) / 4 * 4 - c * kChunkK;
    return (left < kChunkK ? left : kChunkK) / 4;
}
// the first of the kUnitsPerLane units (within a pass) of a wave's half
DRL_LL_HD int lane_unit(int wave, int half) { return (wave * 2 + half) * kUnitsPerLane; }
// words of a policy-code row of a W x W window (drl_policy_code_bytes / 4: 4 groups of cells padded to 8 u16);
// before the first layer the staging area holds the tile's raw code rows (read once, coalesced)
DRL_LL_HD int code_row_words(int W) { return ((W * W + 3) / 4 + 7) / 8 * 8 * 2; }
// thread tid's i-th staged weight (i < kStageLoads): unit (within the pass) and column (within the chunk)
DRL_LL_HD int stage_unit(int tid, int i) { return tid / kChunkK + (kActThreads / kChunkK) * i; }
DRL_LL_HD int stage_k(int tid) { return tid % kChunkK; }

// The act's plan for a validated population plan.  Returns nullptr, or the message for drl_last_error.
inline const char* act_plan(const pop::Plan& p, ActPlan* out) {
    if (!out) return "internal: the league act plan is NULL";
    const ll::Plan& P = p.P;
    *out = ActPlan{};
    out->ldx = odd_quarter(P.in4);
    int widest = 8;
    for (int l = 0; l < P.n_layers; ++l) widest = r8(P.out[l]) > widest ? r8(P.out[l]) : widest;
    out->lda = odd_quarter(widest);
    out->a_floats = kEnvTile * (out->ldx > out->lda ? out->ldx : out->lda);
    out->b_floats = kEnvTile * out->lda;
    out->w_floats = kPassUnits * kChunkK;
    for (int l = 0; l < P.n_layers; ++l)
        if (chunk_quads(P.in[l], chunk_count(P.in[l]) - 1) % 2) return "internal: a layer's last chunk has an odd number of 4-column steps";
    if (kEnvTile * code_row_words(P.code_w) > out->w_floats) return "internal: the tile's code rows exceed the staging area";
    out->lds_bytes = 4 * (out->a_floats + out->b_floats + out->w_floats);
    if (out->lds_bytes > kLdsLimit) return "internal: the league act's LDS plan exceeds a CU's 160 KiB";
    return nullptr;
}

// ---- kernel arguments (dronerl_league.hip; launched by dronerl_league_api.cpp) -------------------------------
struct ActArgs {
    ll::Plan P;
    ActPlan A;
    int32_t members, n_actions;
    int64_t stride;          // bytes from one member block to the next
    const uint8_t* base;
    const uint32_t* codes;   // [n_drones][E][row_words]: drl_obs_code_all's output (learner k reads block k)
    int64_t row_words, E;
    int32_t greedy, n_drones;
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;        // [E][n_drones]: columns 0 .. members - 1 are written
    float* q;                // nullable: [members][E][n_actions]
};

struct AddArgs {
    uint32_t* r_obs;
    uint32_t* r_next;
    int32_t* r_act;
    float* r_rew;
    uint8_t* r_done;
    int64_t capacity, row_words, cursor, E, total;  // total = members * E
    const uint32_t* codes_prev;  // [n_drones][E][row_words]
    const uint32_t* codes;
    const int32_t* actions;      // [E][n_drones]: learner k's column k
    const float* rewards;
    const uint8_t* dones;
    int32_t n_drones;
};

// (hipError_t values)
int launch_league_act(const ActArgs& a, hipStream_t s);
int launch_league_add(const AddArgs& a, hipStream_t s);

}  // namespace league
}  // namespace drl
#endif
