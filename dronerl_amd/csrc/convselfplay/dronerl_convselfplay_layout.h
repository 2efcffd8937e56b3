// dronerl_convselfplay_layout.h — shared-policy self-play for conv learners: K members of a drl_convpop_layout
// block acting in the SAME E envs, learner k on the `team` drone indices drones[k][0 .. team - 1] of every env
// (include/dronerl.h drl_convselfplay_act).  The block, the records, the rings and the learner chain are the conv
// population's (convpop/dronerl_convpop_layout.h), the add is drl_selfplay_replay_add and the act's plan is the
// conv league's (convleague/dronerl_convleague_layout.h: cvl::act_plan), all unchanged; the map's validation and
// the row rule r = j * E + i are selfplay's (selfplay/dronerl_selfplay_layout.h).  This header adds where a tile
// row comes from and goes to, and the kernel's arguments.  Plain C++ (no HIP): the host API, the kernel and
// tests/native/convselfplay_layout_check.cpp share it.
//
// A learner's rows are its team * E (drone, env) pairs flattened slot-major, r = j * E + i.  Workgroup (x, k)
// takes the T = env_tile consecutive rows [T * x, T * x + T) of learner k, so a tile never holds rows of two
// learners but may hold rows of several drones (at E = 1 a team of six is one tile).
#ifndef DRONERL_CONVSELFPLAY_LAYOUT_H
#define DRONERL_CONVSELFPLAY_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"
#include "../convleague/dronerl_convleague_layout.h"
#include "../selfplay/dronerl_selfplay_layout.h"

namespace drl {
namespace cvs {

// workgroups along x for a learner's `rows` rows, and the rows of tile x that exist (the lanes past them hold 0.0
// inputs and store nothing)
DRL_CV_HD int64_t tile_count(int64_t rows, int T) { return (rows + T - 1) / T; }
DRL_CV_HD int tile_rows(int64_t r0, int T, int64_t rows) { return rows - r0 < T ? (int)(rows - r0) : T; }

// The gather's thread map: row_threads(nt, T) threads per tile row (the workgroup is a multiple of 256 threads, T
// at most 16: nt = T * row_threads), thread tid on tile row tid / row_threads, taking that row's cells
// tid % row_threads, + row_threads, ..
DRL_CV_HD int row_threads(int nt, int T) { return nt / T; }

// Row r of learner k's team: its slot and env (selfplay::row_source: one division per row), its drone.
struct RowPlace {
    int32_t j, dr;
    int64_t i;
};
DRL_CV_HD RowPlace place_row(const uint8_t* team_drones /* drones[k] */, int64_t r, int64_t E) {
    const selfplay::RowSource s = selfplay::row_source(r, E);
    return RowPlace{s.j, (int32_t)team_drones[s.j], s.i};
}
// the row's code row in codes [n_drones][E] (in rows), its word of actions [E][n_drones], and the first word of
// its learner's and slot's block of q [members][team][E][n_actions] (the row's Q starts i * n_actions behind it)
DRL_CV_HD int64_t code_row(const RowPlace& p, int64_t E) { return (int64_t)p.dr * E + p.i; }
DRL_CV_HD int64_t action_word(const RowPlace& p, int32_t n_drones) { return p.i * n_drones + p.dr; }
DRL_CV_HD int64_t q_block(int32_t k, int32_t team, const RowPlace& p, int64_t E, int32_t n_actions) {
    return ((int64_t)k * team + p.j) * E * n_actions;
}

// ---- kernel arguments (dronerl_convselfplay.hip; launched by dronerl_convselfplay_api.cpp) -------------------
struct ActArgs {
    cvl::ActArgs c;                    // the conv league act's (c.q: [members][team][E][n_actions])
    int32_t team, rows;                // rows = team * E (< 2^31), a learner's rows
    uint8_t drones[selfplay::kMaxMap]; // [members][team]
};

// (a hipError_t value)
int launch_convselfplay_act(const ActArgs& a, hipStream_t s);

}  // namespace cvs
}  // namespace drl
#endif
