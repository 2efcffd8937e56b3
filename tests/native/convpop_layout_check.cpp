// CPU check of the conv population's block (dronerl_amd/csrc/convpop/dronerl_convpop_layout.h, the header the
// kernels and the host API share).  For three nets (train_jax's default conv net, the sweep's conv 16-32 with
// dense 128-64, a 9x9 two-layer net with stride 2) x members {1, 3} x max_batch {1, 64, 65, 130}:
//   * a member block equals the single agent's (drl::cg::plan at max_batch, which is what
//     drl_convnet_dqn_large_layout_query reports): the public layout, the row's words, the tiles and the partials'
//     place, so a member's slice can be handed to the single-agent code;
//   * the member blocks do not overlap; the stride and every member's start keep 16-byte alignment;
//   * the hyperparameter records sit 16-byte aligned behind the last block, kHRecStride apart, inside `bytes`;
//   * every word of the layout -- the four parameter sets, the counters, the 4096 squared errors, every word of
//     every row below max_batch, every (chunk, parameter) partial, every record -- is placed once over the whole
//     population: a byte map of the allocation counts one writer per byte;
//   * the grids' limits (members in blockIdx.y / z).
// Members 0 and 1025, max_batch 0 and 4097, window 3, an f32-row net, a kernel of 6 and NULL are refused by name.
// Stand-alone host code (no HIP), built and run by tests/test_conv_population.py under the address and
// undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/convpop/dronerl_convpop_layout.h"

using drl::cp::Plan;

struct ConvSpec {
    int co, k, s, p;
};

static drl_convnet_desc make(int W, std::vector<ConvSpec> conv, std::vector<int> dense, int actions = 5,
                             int input = DRL_QNET_INPUT_CODE) {
    drl_convnet_desc d;
    memset(&d, 0, sizeof d);
    d.window = W;
    d.n_conv = (int)conv.size();
    for (size_t i = 0; i < conv.size() && i < 3; ++i) d.conv[i] = {conv[i].co, conv[i].k, conv[i].s, conv[i].p};
    d.n_dense = (int)dense.size();
    for (size_t i = 0; i < dense.size() && i < 2; ++i) d.dense[i] = dense[i];
    d.n_actions = actions;
    d.input = input;
    return d;
}

#define EXPECT(cond)                                    \
    do {                                                \
        if (!(cond)) {                                  \
            printf("  line %d: %s\n", __LINE__, #cond); \
            ++bad;                                      \
        }                                               \
    } while (0)

static int check(const char* name, const drl_convnet_desc& d, int members, int max_batch) {
    std::vector<Plan> holder(1);  // (heap: the sanitizer sees an access past the plan)
    std::vector<drl::cg::Plan> one(1);
    Plan& p = holder[0];
    int bad = 0;
    if (const char* msg = drl::cp::plan(&d, members, max_batch, &p)) {
        printf("%s: refused: %s\n", name, msg);
        return 1;
    }
    if (drl::cg::plan(&d, max_batch, &one[0])) {
        printf("%s: the single agent's plan refuses the net\n", name);
        return 1;
    }
    const drl::cl::Plan& C = p.P.c;
    const drl::cg::Tiles& T = p.P.t;
    // a member block is the single agent's at max_batch
    EXPECT(memcmp(&one[0].c.pub, &C.pub, sizeof C.pub) == 0);
    EXPECT(memcmp(&one[0].t, &T, sizeof T) == 0);
    EXPECT(one[0].c.scratch_words == C.scratch_words && one[0].c.n_params == C.n_params &&
           one[0].c.row_words == C.row_words && one[0].c.rows_off == C.rows_off && one[0].c.sq_off == C.sq_off);
    EXPECT(C.batch == max_batch && p.code_w == d.window && C.code_w == d.window);
    EXPECT(T.chunks == (max_batch + 63) / 64);
    // tiling and alignment
    EXPECT(p.members == members);
    EXPECT(p.stride % 16 == 0 && p.stride >= C.pub.bytes && p.stride < C.pub.bytes + 16);
    EXPECT(p.hp_off == p.stride * members && p.hp_off % 16 == 0);
    EXPECT(p.bytes == p.hp_off + drl::cp::kHRecStride * members);
    EXPECT(drl::cp::kHRecStride >= (int64_t)sizeof(drl::cp::HRec) && drl::cp::kHRecStride % 16 == 0);
    std::vector<uint8_t> map((size_t)p.bytes, 0);
    auto mark = [&](int64_t at, int64_t n) {
        if (at < 0 || at + n > p.bytes) {
            ++bad;
            printf("  out of bounds: %lld + %lld\n", (long long)at, (long long)n);
            return;
        }
        for (int64_t i = 0; i < n; ++i) {
            if (map[(size_t)(at + i)]++) {
                ++bad;
                printf("  byte %lld placed twice\n", (long long)(at + i));
                return;
            }
        }
    };
    for (int m = 0; m < members && bad < 8; ++m) {
        const int64_t b0 = drl::cp::member_off(p, m);
        EXPECT(b0 % 16 == 0 && b0 == p.stride * m);
        EXPECT(b0 + C.pub.bytes <= (m + 1 < members ? drl::cp::member_off(p, m + 1) : p.hp_off));  // (no overlap)
        const int64_t sets[4] = {C.pub.online_off, C.pub.target_off, C.pub.m_off, C.pub.v_off};
        for (int s = 0; s < 4; ++s) mark(b0 + sets[s], C.n_params * 4);
        mark(b0 + C.pub.counters_off, 64);
        const int64_t s0 = b0 + C.pub.scratch_off;
        EXPECT(s0 % 16 == 0);
        mark(s0 + 4 * C.sq_off, 4 * (int64_t)drl::cg::kMaxBatch);
        for (int b = 0; b < max_batch; ++b) mark(s0 + 4 * drl::cl::row_word(C, b, -1, 0, 0), 4 * (int64_t)C.row_words);
        for (int c = 0; c < T.chunks; ++c) mark(s0 + 4 * drl::cg::part_word(C, T, c, 0), 4 * C.n_params);
        // the last word a member's kernels can touch lies inside its block
        EXPECT(C.pub.scratch_off + 4 * (drl::cg::part_word(C, T, T.chunks - 1, C.n_params - 1) + 1) <= C.pub.bytes);
        const int64_t h0 = drl::cp::hrec_off(p, m);
        EXPECT(h0 % 16 == 0 && h0 >= p.stride * members);
        mark(h0, (int64_t)sizeof(drl::cp::HRec));
    }
    // a row's words: the input and every layer's activations and deltas, once, inside the row
    {
        std::vector<char> w((size_t)C.row_words, 0);
        auto take = [&](int at, int n) {
            for (int i = 0; i < n; ++i) {
                if (at + i < 0 || at + i >= C.row_words || w[(size_t)(at + i)]++) {
                    ++bad;
                    printf("  row word %d outside the row or placed twice\n", at + i);
                    return;
                }
            }
        };
        take(0, C.in);
        for (int l = 0; l < C.n_layers; ++l) {
            if (C.l[l].act >= 0) take(C.l[l].act, C.l[l].n_out);
            take(C.l[l].delta, C.l[l].n_out);
        }
        EXPECT(C.row_words * 4 <= drl::cl::kRowLdsMax);
        EXPECT(C.n_actions <= 8 && C.l[C.n_layers - 1].n_out == C.n_actions);  // (the act's Q row)
    }
    // the grids' limits: members in blockIdx.y / z, chunks in blockIdx.y; the workgroups
    EXPECT(members <= 65535 && T.chunks <= 65535);
    EXPECT(T.rows_threads >= 64 && T.rows_threads <= drl::cg::kRowsThreadsMax && T.rows_threads % 64 == 0);
    return bad;
}

static int refused(const drl_convnet_desc* d, int members, int max_batch, const char* word) {
    std::vector<Plan> holder(1);
    const char* msg = drl::cp::plan(d, members, max_batch, &holder[0]);
    if (!msg || !strstr(msg, word)) {
        printf("  expected a refusal naming '%s', got: %s\n", word, msg ? msg : "(accepted)");
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    const struct {
        const char* name;
        drl_convnet_desc d;
    } nets[] = {{"default", make(7, {{8, 3, 1, 1}}, {})},
                {"sweep", make(7, {{16, 3, 1, 1}, {32, 3, 1, 1}}, {128, 64})},
                {"c", make(9, {{8, 3, 1, 0}, {12, 3, 2, 1}}, {16, 8})}};
    for (const auto& n : nets)
        for (int members : {1, 3})
            for (int max_batch : {1, 64, 65, 130}) bad += check(n.name, n.d, members, max_batch);
    bad += check("many", make(5, {{5, 5, 1, 2}}, {128}), 1024, 8);
    const drl_convnet_desc ok = make(7, {{8, 3, 1, 1}}, {});
    bad += refused(&ok, 0, 8, "members");
    bad += refused(&ok, 1025, 8, "members");
    bad += refused(&ok, 4, 0, "max_batch");
    bad += refused(&ok, 4, 4097, "max_batch");
    bad += refused(nullptr, 4, 8, "NULL");
    const drl_convnet_desc w3 = make(3, {{8, 1, 1, 0}}, {}), obs = make(7, {{8, 3, 1, 1}}, {}, 5, DRL_QNET_INPUT_OBS),
                           k6 = make(7, {{8, 6, 1, 1}}, {}), a9 = make(7, {{8, 3, 1, 1}}, {}, 9);
    bad += refused(&w3, 4, 8, "window");
    bad += refused(&obs, 4, 8, "policy code");
    bad += refused(&k6, 4, 8, "kernel_size");
    bad += refused(&a9, 4, 8, "n_actions");
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
