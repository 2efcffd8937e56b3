// CPU check of the conv self-play act's row map (dronerl_amd/csrc/convselfplay/dronerl_convselfplay_layout.h, the
// header the kernel and the host API share).
//   * The grid: env tile T in {16, 8, 4, 2} x envs E in {1, 2, T - 1, T, T + 1, 3 T + 5} x team M in {1, 2, 3, 6} x
//     learners K in {1, 2}, on 13 drones with the permuted map drones[k][j] = (5 (k M + j) + 3) mod 13, 5 actions.
//     The launch is walked as the kernel walks it: workgroup (x, k) for x < tile_count, tile lane t < T, the lane
//     active iff t < tile_rows.  Every row of every learner is taken by exactly one (workgroup, lane); a workgroup's
//     rows are one learner's (they lie in [0, M E) of learner k: no tile holds rows of two learners); the lanes
//     past M E are inactive and their number is tiles x T - M E; the gathered code row of row r, its word of the
//     action matrix and its Q words equal the ones a row-by-row loop over (slot j, env i) gives; no two rows share
//     an action word or a Q word, every one lies inside its buffer, and the columns of drones in no team are never
//     named.
//   * The gather's thread map: for workgroups of 256 .. 1024 threads and every T, over rows of 25, 49 and 81 cells,
//     every (tile row, cell) is taken by exactly one (thread, turn) and a thread stays on one row.
//   * The kernel's argument block fits the 4 KiB a launch can carry.
//   * Which env tiles occur: the conv league checker's descriptor grid (3 windows x one or two conv layers of
//     {1, 8, 32} channels x kernel {1, 3, 5} x stride {1, 2, 3} x padding {0, 1, 2} x four dense tails) plus two
//     9x9 nets of two padded 3x3 layers (16-32 and 32-32 channels) are planned and counted by their tile
//     ("TILES 16:n 8:n 4:n 2:n"); the two nets' tiles are printed for the test that runs them ("NET name : T").
// Stand-alone host code (no HIP), built and run by tests/test_conv_selfplay.py under the address and
// undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/convselfplay/dronerl_convselfplay_layout.h"

using namespace drl::cvs;

#define EXPECT(cond)                                    \
    do {                                                \
        if (!(cond)) {                                  \
            printf("  line %d: %s\n", __LINE__, #cond); \
            ++bad;                                      \
        }                                               \
    } while (0)

struct Conv {
    int c, k, s, p;
};

static drl_convnet_desc desc(int W, const Conv* conv, int n_conv, const int* dense, int n_dense, int actions) {
    drl_convnet_desc d = {};
    d.window = W;
    d.n_conv = n_conv;
    for (int i = 0; i < n_conv; ++i) d.conv[i] = drl_convnet_conv{conv[i].c, conv[i].k, conv[i].s, conv[i].p};
    d.n_dense = n_dense;
    for (int i = 0; i < n_dense; ++i) d.dense[i] = dense[i];
    d.n_actions = actions;
    d.input = DRL_QNET_INPUT_CODE;
    return d;
}

// the env tile of a description, 0 if cg::plan refuses it
static int tile_of(const drl_convnet_desc& d) {
    std::vector<drl::cp::Plan> holder(1);
    drl::cvl::ActPlan A;
    if (drl::cp::plan(&d, 1, 1, &holder[0])) return 0;
    if (drl::cvl::act_plan(holder[0], &A)) return -1;
    return A.env_tile;
}

int main() {
    int bad = 0;
    const int N = 13, NA = 5;
    long cases = 0, straddle = 0, ragged = 0, one_tile_teams = 0;
    const int Ts[] = {16, 8, 4, 2}, Ms[] = {1, 2, 3, 6}, Ks[] = {1, 2};
    for (int T : Ts) {
        const int Es[] = {1, 2, T - 1, T, T + 1, 3 * T + 5};
        for (int E : Es)
            for (int M : Ms)
                for (int K : Ks) {
                    // (the map as the kernel holds it: uint8_t [K][M], checked as the host checks it)
                    int32_t host_map[12];
                    uint8_t map[drl::selfplay::kMaxMap] = {0};
                    for (int e = 0; e < K * M; ++e) map[e] = (uint8_t)(host_map[e] = (5 * e + 3) % N);
                    EXPECT(drl::selfplay::check_map(host_map, K, M, N) == nullptr);
                    const int64_t rows = (int64_t)M * E;
                    // the row-by-row loop
                    std::vector<int64_t> want_src((size_t)(K * rows)), want_act((size_t)(K * rows)), want_q((size_t)(K * rows));
                    for (int k = 0; k < K; ++k) {
                        int64_t r = 0;
                        for (int j = 0; j < M; ++j)
                            for (int i = 0; i < E; ++i, ++r) {
                                const int dr = host_map[k * M + j];
                                want_src[(size_t)(k * rows + r)] = (int64_t)dr * E + i;
                                want_act[(size_t)(k * rows + r)] = (int64_t)i * N + dr;
                                want_q[(size_t)(k * rows + r)] = ((((int64_t)k * M + j) * E) + i) * NA;
                            }
                    }
                    std::vector<int> taken((size_t)(K * rows), 0), act_hits((size_t)(E * N), 0),
                        q_hits((size_t)(K * rows * NA), 0);
                    const int64_t tiles = tile_count(rows, T);
                    EXPECT(tiles >= 1 && (tiles - 1) * T < rows && tiles * T >= rows);
                    long inactive = 0;
                    for (int k = 0; k < K; ++k)
                        for (int64_t x = 0; x < tiles; ++x) {
                            const int64_t r0 = x * T;
                            const int ne = tile_rows(r0, T, rows);
                            EXPECT(ne >= 1 && ne <= T);
                            int first_dr = -1;
                            bool several = false;
                            for (int t = 0; t < T; ++t) {
                                if (t >= ne) {  // a lane past the learner's rows: no row, no store
                                    EXPECT(r0 + t >= rows);
                                    ++inactive;
                                    continue;
                                }
                                const int64_t r = r0 + t;
                                EXPECT(r >= 0 && r < rows);  // (learner k's own rows: no second learner in the tile)
                                if (r < 0 || r >= rows) continue;
                                const RowPlace p = place_row(map + k * M, r, E);
                                EXPECT(p.j >= 0 && p.j < M && p.i >= 0 && p.i < E && (int64_t)p.j * E + p.i == r);
                                EXPECT(p.dr == host_map[k * M + p.j]);
                                ++taken[(size_t)(k * rows + r)];
                                EXPECT(code_row(p, E) == want_src[(size_t)(k * rows + r)]);
                                EXPECT(code_row(p, E) >= 0 && code_row(p, E) < (int64_t)N * E);
                                const int64_t aw = action_word(p, N), qw = q_block(k, M, p, E, NA) + p.i * NA;
                                EXPECT(aw == want_act[(size_t)(k * rows + r)] && qw == want_q[(size_t)(k * rows + r)]);
                                if (aw >= 0 && aw < (int64_t)E * N) ++act_hits[(size_t)aw]; else EXPECT(false);
                                for (int c = 0; c < NA; ++c)
                                    if (qw + c >= 0 && qw + c < K * rows * NA) ++q_hits[(size_t)(qw + c)]; else EXPECT(false);
                                several |= first_dr >= 0 && p.dr != first_dr;
                                first_dr = first_dr < 0 ? p.dr : first_dr;
                            }
                            straddle += several;
                            ragged += ne < T;
                        }
                    EXPECT(inactive == (long)(K * (tiles * T - rows)));
                    for (size_t e = 0; e < taken.size(); ++e) EXPECT(taken[e] == 1);
                    for (size_t e = 0; e < q_hits.size(); ++e) EXPECT(q_hits[e] == 1);
                    // the action matrix: the teams' columns once each, no other column
                    bool in_team[13] = {false};
                    for (int e = 0; e < K * M; ++e) in_team[host_map[e]] = true;
                    for (int i = 0; i < E; ++i)
                        for (int d = 0; d < N; ++d) EXPECT(act_hits[(size_t)(i * N + d)] == (in_team[d] ? 1 : 0));
                    one_tile_teams += E == 1 && M == 6 && T >= 6 && tiles == 1;
                    ++cases;
                    if (bad > 20) {
                        printf("FAILED (%d)\n", bad);
                        return 1;
                    }
                }
    }
    EXPECT(cases == 4 * 6 * 4 * 2 && straddle > 0 && ragged > 0 && one_tile_teams > 0);
    printf("cases %ld: tiles of several drones %ld, ragged tiles %ld, a team of six in one tile %ld\n", cases, straddle,
           ragged, one_tile_teams);
    // the gather's thread map
    for (int nt = drl::cvl::kThreadsMin; nt <= drl::cvl::kThreadsMax; nt += 256)
        for (int T : Ts) {
            const int cell_counts[] = {25, 49, 81};
            for (int cells : cell_counts) {
                const int rt = row_threads(nt, T);
                EXPECT(rt >= 1 && rt * T == nt);
                std::vector<int> hits((size_t)(T * cells), 0);
                for (int tid = 0; tid < nt; ++tid) {
                    const int t = tid / rt;
                    EXPECT(t >= 0 && t < T);
                    for (int c = tid - t * rt; c < cells; c += rt) ++hits[(size_t)(t * cells + c)];
                }
                for (size_t e = 0; e < hits.size(); ++e) EXPECT(hits[e] == 1);
            }
        }
    EXPECT(sizeof(ActArgs) <= 4096);
    printf("kernel arguments %zu bytes\n", sizeof(ActArgs));
    // which env tiles occur
    {
        long by_tile[17] = {0}, refused = 0;
        const int cs[] = {1, 8, 32}, ks[] = {1, 3, 5}, ss[] = {1, 2, 3}, ps[] = {0, 1, 2};
        const int dense[4][2] = {{0, 0}, {8, 0}, {128, 0}, {128, 64}};
        const int n_dense[4] = {0, 1, 1, 2};
        std::vector<Conv> one;
        for (int c : cs)
            for (int k : ks)
                for (int s : ss)
                    for (int p : ps) one.push_back(Conv{c, k, s, p});
        for (int W = 5; W <= 9; W += 2)
            for (int nc = 1; nc <= 2; ++nc)
                for (size_t i = 0; i < one.size(); ++i)
                    for (size_t j = 0; j < (nc == 2 ? one.size() : 1); ++j)
                        for (int dn = 0; dn < 4; ++dn) {
                            const Conv conv[2] = {one[i], one[j]};
                            const int T = tile_of(desc(W, conv, nc, dense[dn], n_dense[dn], 5));
                            EXPECT(T >= 0);
                            if (T > 0) ++by_tile[T]; else ++refused;
                        }
        const Conv n8[2] = {{16, 3, 1, 1}, {32, 3, 1, 1}}, n4[2] = {{32, 3, 1, 1}, {32, 3, 1, 1}};
        const int none[2] = {0, 0};
        const int t8 = tile_of(desc(9, n8, 2, none, 0, 5)), t4 = tile_of(desc(9, n4, 2, none, 0, 5));
        EXPECT(t8 > 0 && t4 > 0);
        if (t8 > 0) ++by_tile[t8];
        if (t4 > 0) ++by_tile[t4];
        printf("NET 9x9-16-32 : %d\nNET 9x9-32-32 : %d\n", t8, t4);
        printf("TILES 16:%ld 8:%ld 4:%ld 2:%ld (refused %ld)\n", by_tile[16], by_tile[8], by_tile[4], by_tile[2], refused);
    }
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
