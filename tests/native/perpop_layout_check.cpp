// CPU check of the prioritized population's device block (dronerl_amd/csrc/perpop/dronerl_perpop_layout.h, the
// header the kernels and the host API share).  For (members, capacity, max_batch) in (1, 1, 1), (3, 257, 65),
// (4, 5000, 1030), (256, 100000, 256) and (1024, 100000, 4096):
//   * a member's plan equals per::plan(capacity, max_batch) field for field; the stride and the records' offset
//     are multiples of 16;
//   * every byte of every member belongs to exactly one field (a field's region runs to the next field's start: its
//     bytes and at most 15 of padding), member blocks do not overlap each other, and the records lie behind the
//     last block, 32 bytes each, inside `bytes` -- as intervals for every case, and byte by byte on a map of the
//     whole block for the cases that fit in 64 MB;
//   * the rebuild's launches with the member in the grid: workgroup (g, m) of a launch touches only nodes of
//     member m's tree.
// Members 0 and 1025, capacities 0 and 2^24 + 1 and max_batch 0 and 4097 must be refused by name.  Stand-alone host
// code (no HIP), built and run by tests/test_population_per.py under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/perpop/dronerl_perpop_layout.h"

using namespace drl::perpop;

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("  line %d: %s\n", __LINE__, #cond);           \
            ++bad;                                                \
        }                                                         \
    } while (0)

static int check(int32_t members, int64_t capacity, int32_t max_batch) {
    std::vector<Plan> holder(1);  // (heap: the sanitizer sees an access past the plan)
    Plan& p = holder[0];
    int bad = 0;
    if (const char* msg = plan(members, capacity, max_batch, &p)) {
        printf("members %d capacity %lld max_batch %d: refused: %s\n", members, (long long)capacity, max_batch, msg);
        return 1;
    }
    drl::per::Plan one;
    EXPECT(drl::per::plan(capacity, max_batch, &one) == nullptr);
    EXPECT(memcmp(&one.pub, &p.T.pub, sizeof one.pub) == 0);
    EXPECT(one.P == p.T.P && one.logP == p.T.logP && one.capacity == p.T.capacity && one.batch == p.T.batch);
    EXPECT(p.members == members && p.max_batch == max_batch);
    const drl_per_layout& o = p.T.pub;
    const int64_t P = p.T.P;
    const int64_t off[7] = {o.tree_off, o.pmax_off, o.wmax_off, o.slots_off, o.weights_off, o.absd_off, o.bytes};
    const int64_t need[6] = {2 * P * 4, 4, 4, (int64_t)max_batch * 8, (int64_t)max_batch * 4, (int64_t)max_batch * 4};
    EXPECT(off[0] == 0);
    for (int i = 0; i < 6; ++i) {
        EXPECT(off[i] % 16 == 0);
        EXPECT(off[i] + need[i] <= off[i + 1]);     // the field fits before the next one
        EXPECT(off[i + 1] - off[i] < need[i] + 16);  // and nothing but padding lies between them
    }
    EXPECT(p.stride % 16 == 0 && p.stride >= o.bytes && p.stride < o.bytes + 16);
    EXPECT(p.hp_off % 16 == 0 && p.hp_off == p.stride * members);
    EXPECT(kPRecStride % 16 == 0 && kPRecStride >= (int64_t)sizeof(PRec));
    EXPECT(p.bytes == p.hp_off + kPRecStride * members);
    for (int m = 0; m < members; ++m) {
        EXPECT(member_off(p, m) == p.stride * m && member_off(p, m) + o.bytes <= p.hp_off);
        EXPECT(m == 0 || member_off(p, m - 1) + o.bytes <= member_off(p, m));
        EXPECT(prec_off(p, m) >= p.hp_off && prec_off(p, m) + (int64_t)sizeof(PRec) <= p.bytes);
        EXPECT(m == 0 || prec_off(p, m - 1) + (int64_t)sizeof(PRec) <= prec_off(p, m));
    }
    if (p.bytes <= ((int64_t)64 << 20)) {  // byte by byte
        std::vector<uint8_t> owner((size_t)p.bytes, 0);
        for (int m = 0; m < members; ++m) {
            for (int i = 0; i < 6; ++i)
                for (int64_t b = off[i]; b < off[i + 1]; ++b) ++owner[(size_t)(member_off(p, m) + b)];
            for (int64_t b = member_off(p, m) + o.bytes; b < member_off(p, m) + p.stride; ++b) ++owner[(size_t)b];
            for (int64_t b = 0; b < kPRecStride; ++b) ++owner[(size_t)(prec_off(p, m) + b)];
        }
        for (int64_t b = 0; b < p.bytes; ++b)
            if (owner[(size_t)b] != 1) {
                printf("  byte %lld owned %d times\n", (long long)b, (int)owner[(size_t)b]);
                ++bad;
                break;
            }
    }
    // the rebuild with the member in the grid: the nodes workgroup (g, m) reads and writes, as block offsets
    const int64_t run = drl::per::rebuild_run(P), groups = drl::per::rebuild_groups(P);
    EXPECT(run * groups == P && run <= drl::per::kRun && groups <= drl::per::kRun);
    const int ms[3] = {0, members / 2, members - 1};
    for (int m : ms) {
        const int64_t lo = member_off(p, m) + o.tree_off, hi = lo + 2 * P * 4;
        const int64_t launches[2][3] = {{groups, groups, run}, {1, 1, groups}};  // root0, workgroups, n
        for (int k = 0; k < 2; ++k) {
            if ((k == 0 && run <= 1) || (k == 1 && groups <= 1)) continue;
            const int64_t root0 = launches[k][0], wgs = launches[k][1], n = launches[k][2];
            for (int64_t g = 0; g < wgs; g += (wgs > 2 ? wgs - 1 : 1)) {  // the first and the last workgroup
                const int64_t first = (root0 + g) * n, last = (root0 + g + 1) * n - 1;  // the leaves' level
                EXPECT(lo + first * 4 >= lo + 4 && lo + last * 4 + 4 <= hi);
                EXPECT(root0 + g >= 1);  // the subtree's root, the smallest node written
            }
        }
    }
    if (bad) printf("members %d capacity %lld max_batch %d: %d failures\n", members, (long long)capacity, max_batch, bad);
    return bad;
}

int main() {
    int bad = 0;
    bad += check(1, 1, 1);
    bad += check(3, 257, 65);
    bad += check(4, 5000, 1030);
    bad += check(256, 100000, 256);
    bad += check(1024, 100000, 4096);
    bad += check(2, (int64_t)1 << 24, 4096);
    Plan p;
    const char* m;
    m = plan(0, 100, 8, &p);
    EXPECT(m && strstr(m, "members must be in [1, 1024]"));
    m = plan(1025, 100, 8, &p);
    EXPECT(m && strstr(m, "members must be in [1, 1024]"));
    m = plan(4, 0, 8, &p);
    EXPECT(m && strstr(m, "capacity must be in [1, 2^24]"));
    m = plan(4, ((int64_t)1 << 24) + 1, 8, &p);
    EXPECT(m && strstr(m, "capacity must be in [1, 2^24]"));
    m = plan(4, 100, 0, &p);
    EXPECT(m && strstr(m, "max_batch must be in [1, 4096]"));
    m = plan(4, 100, 4097, &p);
    EXPECT(m && strstr(m, "max_batch must be in [1, 4096]"));
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
