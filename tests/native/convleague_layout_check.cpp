// CPU check of the conv league act's plan (dronerl_amd/csrc/convleague/dronerl_convleague_layout.h, the header
// the kernel and the host API share).  The descriptors: for each code window (5x5, 7x7, 9x9)
//   * the nets of tests/_conv_learner_ref.py NETS that read the code (a, b, c, f, g, h, i), each at its window;
//   * the grid: 1 or 2 conv layers, each of {1, 8, 32} out channels x kernel {1, 3, 5} x stride {1, 2, 3} x
//     padding {0, 1, 2}, followed by the dense widths {}, {8}, {128} or {128, 64}, with 5 actions:
//     3 windows x (81 + 81^2) x 4 = 79,704 descriptions, of which cg::plan accepts the ones counted below (it
//     refuses a kernel larger than the padded map and a learner row above 64 KB).
// For every accepted descriptor
//   * the plan exists, its LDS is env_tile x row_words x 4 bytes and stays within kLdsLimit (160 KiB);
//   * env_tile is one of kEnvTiles and the largest that fits; env_tile = 2 is never refused;
//   * the forward-only row is no larger than the learner's row (cl::Plan::row_words), and over the tile's rows
//     every input word, every layer's output word and the head's words are placed exactly once: nothing overlaps
//     inside a row or between envs, nothing lies outside the LDS, a layer reads what the layer before wrote, and
//     the words nothing is placed on are the pads that round a region up to 4 words;
//   * the workgroup is a multiple of 256 threads in [256, 1024].
// Prints the plan of the named nets ("PLAN name : env_tile threads row_words lds_bytes") for the test that
// compares them with what the Python layer reads.  Stand-alone host code (no HIP), built and run by
// tests/test_conv_league.py under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/convleague/dronerl_convleague_layout.h"

using namespace drl::cvl;

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

static int worst = 0;

// 0: accepted and checked (bad += failures); 1: cg::plan refuses the description
static int check(const drl_convnet_desc& d, const char* name, int& bad, bool must_accept) {
    std::vector<drl::cp::Plan> holder(1);
    std::vector<ActPlan> aholder(2);
    drl::cp::Plan& p = holder[0];
    ActPlan& A = aholder[0];
    if (const char* msg = drl::cp::plan(&d, 1, 1, &p)) {
        if (must_accept) {
            printf("net %s refused: %s\n", name, msg);
            ++bad;
        }
        return 1;
    }
    if (const char* msg = act_plan(p, &A)) {
        printf("no act plan: %s\n", msg);
        ++bad;
        return 0;
    }
    const drl::cl::Plan& P = p.P.c;
    const int T = A.env_tile, S = A.row_words;
    EXPECT(A.lds_bytes == T * S * 4 && A.lds_bytes <= kLdsLimit && kLdsLimit == 160 * 1024);
    EXPECT(S % 4 == 0 && S <= P.row_words && A.n_layers == P.n_layers);
    EXPECT(A.threads % 256 == 0 && A.threads >= kThreadsMin && A.threads <= kThreadsMax);
    // T: in the list, and the largest that fits
    int at = -1;
    for (int i = 0; i < kNumEnvTiles; ++i) {
        EXPECT(i == 0 ? kEnvTiles[i] == kMaxEnvTile : kEnvTiles[i] < kEnvTiles[i - 1]);
        if (kEnvTiles[i] == T) at = i;
    }
    EXPECT(at >= 0);
    for (int i = 0; i < at; ++i) {
        EXPECT((int64_t)kEnvTiles[i] * S * 4 > kLdsLimit);
        EXPECT(act_plan_for(P, kEnvTiles[i], &aholder[1]) != nullptr);
    }
    EXPECT(act_plan_for(P, 2, &aholder[1]) == nullptr && aholder[1].row_words == S);
    // the rows: every word once
    std::vector<int> word((size_t)T * (size_t)S, 0);
    auto place = [&](int r, int w) {
        const int at_ = lds_word(A, r, w);
        if (w < 0 || w >= S || at_ < 0 || at_ >= T * S) {
            ++bad;
            printf("  row %d word %d outside the LDS\n", r, w);
        } else {
            ++word[(size_t)at_];
        }
    };
    int64_t placed = 0;
    for (int r = 0; r < T; ++r) {
        for (int i = 0; i < P.in; ++i) place(r, in_word(A, 0) + i);
        placed += P.in;
        for (int l = 0; l < P.n_layers; ++l) {
            for (int e = 0; e < P.l[l].n_out; ++e) place(r, A.out[l] + e);
            placed += P.l[l].n_out;
            // a layer reads what the layer before wrote
            EXPECT(in_word(A, l) == (l == 0 ? 0 : A.out[l - 1]));
            EXPECT(P.l[l].n_in == (l == 0 ? P.in : P.l[l - 1].n_out));
            EXPECT(A.out[l] % 4 == 0);
            EXPECT(A.out[l] - (l == 0 ? P.in : A.out[l - 1] + P.l[l - 1].n_out) < 4);
        }
        EXPECT(S - (A.out[P.n_layers - 1] + P.l[P.n_layers - 1].n_out) < 4);
    }
    int64_t once = 0, never = 0;
    for (size_t i = 0; i < word.size(); ++i) {
        once += word[i] == 1;
        never += word[i] == 0;
    }
    EXPECT(once == placed && once + never == (int64_t)word.size());
    EXPECT(P.l[P.n_layers - 1].n_out == P.n_actions && P.n_actions <= 8);
    worst = A.lds_bytes > worst ? A.lds_bytes : worst;
    if (name) printf("PLAN %s : %d %d %d %d\n", name, T, A.threads, S, A.lds_bytes);
    return 0;
}

int main() {
    int bad = 0;
    long tried = 0, accepted = 0;
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
                        ++tried;
                        accepted += 1 - check(desc(W, conv, nc, dense[dn], n_dense[dn], 5), nullptr, bad, false);
                        if (bad > 20) {
                            printf("FAILED (%d)\n", bad);
                            return 1;
                        }
                    }
    printf("grid %ld, accepted %ld, the largest LDS plan %d of %d bytes\n", tried, accepted, worst, kLdsLimit);
    // tests/_conv_learner_ref.py NETS on the code (e has a 3x3 window: f32 rows only)
    struct Net {
        const char* name;
        int W, nc;
        Conv conv[3];
        int nd, dense[2];
    };
    const Net nets[] = {
        {"a", 7, 1, {{4, 3, 1, 1}}, 1, {8, 0}},
        {"b", 7, 1, {{8, 3, 1, 1}}, 0, {0, 0}},
        {"c", 9, 2, {{8, 3, 1, 0}, {12, 3, 2, 1}}, 2, {16, 8}},
        {"f", 7, 1, {{6, 2, 3, 0}}, 0, {0, 0}},
        {"g", 5, 1, {{5, 5, 1, 2}}, 1, {128, 0}},
        {"h", 9, 3, {{8, 3, 1, 1}, {8, 3, 2, 0}, {16, 2, 1, 0}}, 0, {0, 0}},
        {"i", 7, 2, {{5, 3, 1, 1}, {7, 2, 3, 0}}, 1, {8, 0}},
    };
    for (const Net& n : nets) check(desc(n.W, n.conv, n.nc, n.dense, n.nd, 5), n.name, bad, true);
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
