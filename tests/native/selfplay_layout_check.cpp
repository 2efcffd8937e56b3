// CPU check of the self-play row map (dronerl_amd/csrc/selfplay/dronerl_selfplay_layout.h, the header the kernels
// and the host API share).
//   * For capacity in {5, 8, 24}, E in {1, 2, 4, 9}, team M in {1, 2, 3} and several cursors: the slots ring_slot
//     gives the rows row_kept keeps equal a ring that ReplayBuffer.add_many's rule fills with the M * E rows one by
//     one (row r = j * E + i carries the tag (j, i) that row_source gives it).  The cases hold M * E < capacity
//     with a wrap, M * E == capacity, M * E > capacity with E < capacity (the cut falls inside a team slot) and
//     E > capacity; each class is counted and must occur.
//   * row_source inverts r = j * E + i, also past 2^31.
//   * check_map accepts the default, permuted and non-contiguous maps and refuses NULL, team < 1,
//     members * team > n_drones, an index outside [0, n_drones) and an index named twice.
// Stand-alone host code (no HIP), built and run by tests/test_selfplay.py under the address and
// undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/selfplay/dronerl_selfplay_layout.h"

using namespace drl::selfplay;

#define EXPECT(cond)                                    \
    do {                                                \
        if (!(cond)) {                                  \
            printf("  line %d: %s\n", __LINE__, #cond); \
            ++bad;                                      \
        }                                               \
    } while (0)

static bool refused(const char* msg, const char* word) { return msg && strstr(msg, word); }

int main() {
    int bad = 0;
    long cases = 0, wraps = 0, equal = 0, cut_inside = 0, e_above = 0;
    const int caps[] = {5, 8, 24}, envs[] = {1, 2, 4, 9}, teams[] = {1, 2, 3};
    for (int cap : caps)
        for (int E : envs)
            for (int M : teams)
                for (int cursor = 0; cursor < cap; cursor += (cap > 8 ? 5 : 1)) {
                    const int total = M * E;
                    // the reference: add_many's rule, the rows one by one (a row is its tag j * 16 + i, + 1)
                    std::vector<int> want((size_t)cap, 0), got((size_t)cap, 0), writes((size_t)cap, 0);
                    {
                        int cur = cursor;
                        for (int j = 0; j < M; ++j)
                            for (int i = 0; i < E; ++i) {
                                want[(size_t)cur] = j * 16 + i + 1;
                                cur = (cur + 1) % cap;
                            }
                    }
                    for (int64_t r = 0; r < total; ++r) {
                        const RowSource s = row_source(r, E);
                        EXPECT(s.j >= 0 && s.j < M && s.i >= 0 && s.i < E && (int64_t)s.j * E + s.i == r);
                        if (!row_kept(r, total, cap)) continue;
                        const int64_t slot = ring_slot(cursor, r, cap);
                        EXPECT(slot >= 0 && slot < cap);
                        if (slot < 0 || slot >= cap) continue;
                        got[(size_t)slot] = s.j * 16 + (int)s.i + 1;
                        ++writes[(size_t)slot];
                    }
                    for (int s = 0; s < cap; ++s) {
                        EXPECT(got[(size_t)s] == want[(size_t)s]);
                        EXPECT(writes[(size_t)s] <= 1);  // (no two threads store to one slot)
                    }
                    ++cases;
                    wraps += total < cap && cursor + total > cap;
                    equal += total == cap;
                    cut_inside += total > cap && E < cap && (total - cap) % E != 0;
                    e_above += E > cap;
                    if (bad > 20) {
                        printf("FAILED (%d)\n", bad);
                        return 1;
                    }
                }
    EXPECT(wraps > 0 && equal > 0 && cut_inside > 0 && e_above > 0);
    printf("cases %ld: wraps %ld, equal %ld, cut inside a slot %ld, E above capacity %ld\n", cases, wraps, equal,
           cut_inside, e_above);
    // row_source past 2^31
    {
        const int64_t E = ((int64_t)1 << 31) + 7, r = 3 * E + 5;
        const RowSource s = row_source(r, E);
        EXPECT(s.j == 3 && s.i == 5);
    }
    // the map
    {
        const int32_t ident[6] = {0, 1, 2, 3, 4, 5}, perm[4] = {4, 0, 3, 1}, desc3[3] = {4, 2, 0};
        EXPECT(!check_map(ident, 1, 6, 6) && !check_map(ident, 6, 1, 6) && !check_map(ident, 2, 3, 6) && !check_map(ident, 3, 2, 64));
        EXPECT(!check_map(perm, 2, 2, 5) && !check_map(perm, 1, 4, 5) && !check_map(desc3, 1, 3, 5));
        EXPECT(refused(check_map(nullptr, 1, 1, 4), "NULL"));
        EXPECT(refused(check_map(ident, 1, 0, 4), "team") && refused(check_map(ident, 1, -2, 4), "team"));
        EXPECT(refused(check_map(ident, 2, 3, 5), "members * team") && refused(check_map(ident, 0, 1, 5), "members * team"));
        EXPECT(refused(check_map(ident, 1 << 20, 1 << 20, 5), "members * team"));  // (no 32-bit overflow)
        EXPECT(refused(check_map(ident, 1, 1, 65), "members * team"));
        EXPECT(refused(check_map(perm, 2, 2, 4), "outside"));
        const int32_t neg[2] = {1, -1}, dup[4] = {0, 2, 3, 2};
        EXPECT(refused(check_map(neg, 1, 2, 4), "outside"));
        EXPECT(refused(check_map(dup, 2, 2, 4), "twice") && refused(check_map(dup, 1, 4, 4), "twice"));
        EXPECT(!check_map(dup, 1, 3, 4));  // (the entries past members * team are not read)
    }
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
