// CPU check of the prioritized replay's device block (dronerl_amd/csrc/per/dronerl_per_layout.h, the header the
// kernels and the host API share).  For capacities 1, 2, 3, 255, 256, 257, 4096, 4097, 5000, 100,000 and 2^24 and
// batches 1, 65 and 4096:
//   * P is the smallest power of two >= capacity and logP its logarithm; the tree, pmax, wmax, the slots, the
//     weights and |d| tile [0, bytes) without overlap, each on a 16-byte boundary;
//   * the rebuild's launches, run here on a host array with the kernel's index rule (workgroup g of launch k owns
//     the subtree of `run` leaves rooted at node root0 + g; the level of w nodes is the tree's [root * w,
//     (root + 1) * w)): every internal node is written exactly once, from children that are leaves or were written
//     before it, no index leaves [1, 2P), and the result equals the plain bottom-up tree bit for bit.
// Capacities 0 and 2^24 + 1 and batches 0 and 4097 must be refused by name.  Stand-alone host code (no HIP), built
// and run by tests/test_prioritized_replay.py under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/per/dronerl_per_layout.h"

using namespace drl::per;

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("  line %d: %s\n", __LINE__, #cond);           \
            ++bad;                                                \
        }                                                         \
    } while (0)

static uint32_t rng_state = 12345u;
static float next_leaf() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f) + 1e-3f;
}

// one launch of the rebuild kernel: `groups` workgroups over subtrees of n leaves rooted at root0 + g
static int run_launch(std::vector<float>& tree, std::vector<uint8_t>& written, int64_t P, int64_t root0, int64_t groups,
                      int64_t n) {
    int bad = 0;
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t root = root0 + g;
        std::vector<float> heap(2 * n, 0.0f);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t node = root * n + i;
            EXPECT(node >= 1 && node < 2 * P);
            EXPECT(node >= P || written[node] == 1);  // a leaf, or a node an earlier launch wrote
            heap[n + i] = tree[node];
        }
        for (int64_t w = n >> 1; w >= 1; w >>= 1)
            for (int64_t i = 0; i < w; ++i) {
                const float v = heap[2 * (w + i)] + heap[2 * (w + i) + 1];
                heap[w + i] = v;
                const int64_t node = root * w + i;
                EXPECT(node >= 1 && node < P);
                ++written[node];
                tree[node] = v;
            }
    }
    return bad;
}

static int check(int64_t capacity, int32_t batch) {
    std::vector<Plan> holder(1);  // (heap: the sanitizer sees an access past the plan)
    Plan& p = holder[0];
    int bad = 0;
    if (const char* msg = plan(capacity, batch, &p)) {
        printf("capacity %lld batch %d: refused: %s\n", (long long)capacity, batch, msg);
        return 1;
    }
    const int64_t P = p.P;
    EXPECT(P >= capacity && (P & (P - 1)) == 0 && (P == 1 || P / 2 < capacity));
    EXPECT(((int64_t)1 << p.logP) == P);
    const drl_per_layout& o = p.pub;
    EXPECT(o.capacity == capacity && o.leaves == P && o.batch == batch);
    const int64_t off[7] = {o.tree_off, o.pmax_off, o.wmax_off, o.slots_off, o.weights_off, o.absd_off, o.bytes};
    const int64_t need[6] = {2 * P * 4, 4, 4, (int64_t)batch * 8, (int64_t)batch * 4, (int64_t)batch * 4};
    EXPECT(off[0] == 0);
    for (int i = 0; i < 6; ++i) {
        EXPECT(off[i] % 16 == 0);
        EXPECT(off[i] + need[i] <= off[i + 1]);
        EXPECT(off[i + 1] - off[i] < need[i] + 16);
    }
    EXPECT(o.bytes % 16 == 0);
    // the rebuild on a host tree
    std::vector<float> tree(2 * P, 0.0f), want(2 * P, 0.0f);
    std::vector<uint8_t> written(2 * P, 0);
    for (int64_t s = 0; s < capacity; ++s)
        if (s % 7 != 3) tree[P + s] = want[P + s] = next_leaf();  // (some slots never written)
    for (int64_t i = P - 1; i >= 1; --i) want[i] = want[2 * i] + want[2 * i + 1];
    for (int64_t i = 1; i < P; ++i) tree[i] = -1.0f;  // stale internal nodes
    const int64_t run = rebuild_run(P), groups = rebuild_groups(P);
    EXPECT(run >= 1 && run <= kRun && groups >= 1 && groups <= kRun && run * groups == P);
    EXPECT(groups == 1 || run == kRun);
    if (run > 1) bad += run_launch(tree, written, P, groups, groups, run);
    if (groups > 1) bad += run_launch(tree, written, P, 1, 1, groups);
    for (int64_t i = 1; i < P; ++i) {
        if (written[i] != 1 || memcmp(&tree[i], &want[i], 4)) {
            printf("  node %lld: written %d times, %a want %a\n", (long long)i, (int)written[i], tree[i], want[i]);
            ++bad;
            break;
        }
    }
    if (bad) printf("capacity %lld batch %d: %d failures\n", (long long)capacity, batch, bad);
    return bad;
}

int main() {
    int bad = 0;
    const int64_t caps[] = {1, 2, 3, 255, 256, 257, 4096, 4097, 5000, 100000, (int64_t)1 << 24};
    const int32_t batches[] = {1, 65, 4096};
    for (int64_t c : caps)
        for (int32_t b : batches)
            if (c <= 100000 || b == 4096) bad += check(c, b);  // (the largest tree once: 2^25 nodes)
    Plan p;
    const char* m;
    m = plan(0, 8, &p);
    EXPECT(m && strstr(m, "capacity must be in [1, 2^24]"));
    m = plan(((int64_t)1 << 24) + 1, 8, &p);
    EXPECT(m && strstr(m, "capacity must be in [1, 2^24]"));
    m = plan(100, 0, &p);
    EXPECT(m && strstr(m, "batch must be in [1, 4096]"));
    m = plan(100, 4097, &p);
    EXPECT(m && strstr(m, "batch must be in [1, 4096]"));
    EXPECT(leaves_of(100000) == 131072 && leaves_of(1) == 1 && leaves_of(257) == 512);
    static_assert(kSampleThreads * kSampleRows == kMaxBatch, "a sample workgroup's threads cover the largest batch");
    static_assert(kTop % 2 == 0 && kTop * 4 + 2 * kRun * 4 <= 64 * 1024, "the kernels' static LDS");
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
