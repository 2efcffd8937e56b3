// dronerl_selfplay_layout.h — shared-policy self-play: K learners ("members" of a drl_pop_layout block) acting in
// the SAME E envs, learner k on the `team` drone indices drones[k][0 .. team - 1] of every env
// (include/dronerl.h drl_selfplay_*).  The block, the records and the rings are the population's, unchanged; the
// act's plan and tiling are the league's (league/dronerl_league_layout.h), unchanged.  This header adds the map
// from a learner's rows to (team slot, env), the rings' slot rule and the two kernels' arguments.  Plain C++ (no
// HIP): the host API, the kernels and tests/native/selfplay_layout_check.cpp share it.
//
// A learner's rows are its team * E (drone, env) pairs flattened slot-major, r = j * E + i: the act takes 32
// consecutive r per workgroup (a tile may hold rows of several drones: at E = 1 a team of six is one tile), and
// the add lands row r where ReplayBuffer.add_many would land the r-th of team * E rows added one by one.
#ifndef DRONERL_SELFPLAY_LAYOUT_H
#define DRONERL_SELFPLAY_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../league/dronerl_league_layout.h"

namespace drl {
namespace selfplay {

constexpr int kMaxMap = DRL_MAX_DRONES;  // members * team <= n_drones <= 64: the map travels by value
static_assert(kMaxMap == 64 && DRL_MAX_DRONES <= 256, "a map entry is a uint8_t, the map is uint8_t[64]");

// The map's validation: nullptr, or the message for drl_last_error.  drones: HOST [members][team].
inline const char* check_map(const int32_t* drones, int32_t members, int32_t team, int32_t n_drones) {
    if (!drones) return "drones (the host map [members][team]) is NULL";
    if (team < 1) return "team must be >= 1: the drone indices a learner drives";
    if (members < 1 || (int64_t)members * team > n_drones || n_drones > kMaxMap)
        return "members * team must be in [1, n_drones]: a drone index has at most one learner";
    bool seen[kMaxMap] = {false};
    for (int e = 0; e < members * team; ++e) {
        if (drones[e] < 0 || drones[e] >= n_drones) return "drones: an index outside [0, n_drones)";
        if (seen[drones[e]]) return "drones: a drone index is named twice";
        seen[drones[e]] = true;
    }
    return nullptr;
}

// row r of a learner -> (team slot j, env i): r = j * E + i
struct RowSource {
    int32_t j;
    int64_t i;
};
DRL_LL_HD RowSource row_source(int64_t r, int64_t E) {
    const int64_t j = r / E;
    return RowSource{(int32_t)j, r - j * E};
}
// add_many on a learner's `total` = team * E rows: row r lands in slot (cursor + r) % capacity, and with
// total > capacity only the last `capacity` rows are stored
DRL_LL_HD int64_t ring_slot(int64_t cursor, int64_t r, int64_t capacity) { return (cursor + r) % capacity; }
DRL_LL_HD bool row_kept(int64_t r, int64_t total, int64_t capacity) { return r >= total - capacity; }

// ---- kernel arguments (dronerl_selfplay.hip; launched by dronerl_selfplay_api.cpp) ---------------------------
struct ActArgs {
    ll::Plan P;
    league::ActPlan A;
    int32_t members, n_actions;
    int64_t stride;          // bytes from one member block to the next
    const uint8_t* base;
    const uint32_t* codes;   // [n_drones][E][row_words]: drl_obs_code_all's output
    int64_t row_words, E;
    int32_t greedy, n_drones;
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;        // [E][n_drones]: the teams' columns are written
    float* q;                // nullable: [members][team][E][n_actions]
    int32_t team, rows;      // rows = team * E (< 2^31), a learner's rows
    uint8_t drones[kMaxMap]; // [members][team]
};

struct AddArgs {
    uint32_t* r_obs;
    uint32_t* r_next;
    int32_t* r_act;
    float* r_rew;
    uint8_t* r_done;
    int64_t capacity, row_words, cursor, E, rows, total;  // rows = team * E, total = members * rows
    const uint32_t* codes_prev;  // [n_drones][E][row_words]
    const uint32_t* codes;
    const int32_t* actions;      // [E][n_drones]
    const float* rewards;
    const uint8_t* dones;
    int32_t n_drones, team;
    uint8_t drones[kMaxMap];
};

// (hipError_t values)
int launch_selfplay_act(const ActArgs& a, hipStream_t s);
int launch_selfplay_add(const AddArgs& a, hipStream_t s);

}  // namespace selfplay
}  // namespace drl
#endif
