// CPU check of the league act's plan (dronerl_amd/csrc/league/dronerl_league_layout.h, the header the kernel and
// the host API share).  For EVERY descriptor the population accepts -- windows 5x5, 7x7 and 9x9; 1, 2 or 3 hidden
// widths, each a multiple of 8 up to DRL_WIDENET_MAX_WIDTH; 1..8 actions: 811,776 of them --
//   * the LDS of a launch (two row regions and the staged weight chunk) stays within kLdsLimit, the regions are
//     16-byte aligned and hold every layer's rows: a layer's input region never is its output region;
//   * the row strides are multiples of 4 floats with an odd quarter (the 16 lanes a 16-byte read serves together,
//     16 different envs, fall on 16 different 16-byte bank groups: checked by counting), and hold every input
//     and every 4-unit store;
//   * the passes, waves, halves and a lane's units cover every unit of every layer exactly once, and the chunks'
//     4-column steps cover every input exactly once and stop at the zero pad (never past the row);
//   * the staging map writes every word of the weight chunk exactly once, and the tile's raw code rows fit the
//     staging area.
// The two counting checks of a layer (units, inputs) depend on the layer's (inputs, units) pair alone: they run
// on every net of 1 or 2 hidden layers, which hold every such pair, and on a 3-layer net in 16; everything else
// runs on every descriptor.
// Prints the plan of a few nets ("PLAN in h0 h1 h2 actions : env_tile ldx lda lds_bytes") for the test that
// compares them with what the Python layer reads.  Stand-alone host code (no HIP), built and run by
// tests/test_league.py under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/league/dronerl_league_layout.h"

using namespace drl::league;

#define EXPECT(cond)                                    \
    do {                                                \
        if (!(cond)) {                                  \
            printf("  line %d: %s\n", __LINE__, #cond); \
            ++bad;                                      \
        }                                               \
    } while (0)

static drl_widenet_desc desc(int in, const int* hidden, int n_hidden, int actions) {
    drl_widenet_desc d = {};
    d.in_features = in;
    d.n_hidden = n_hidden;
    for (int i = 0; i < n_hidden; ++i) d.hidden[i] = hidden[i];
    d.n_actions = actions;
    d.input = DRL_QNET_INPUT_CODE;
    return d;
}

// the 16 lanes one ds_read_b128 cycle serves (MI355X: {0-3, 12-15, 20-27} and its three images)
static const int kGroup[16] = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27};

static int stride_ok(int ld) {
    int seen[16] = {0};
    for (int i = 0; i < 16; ++i) {
        const int env = kGroup[i] & (kEnvTile - 1);
        const int slot = (env * ld / 4) % 16;  // the 16-byte bank group of the env's row at any 16-byte column
        if (seen[slot]++) return 0;
    }
    return ld % 4 == 0;
}

static int check(const drl_widenet_desc& d, bool print, bool count = true) {
    std::vector<drl::pop::Plan> holder(1);
    std::vector<ActPlan> aholder(1);
    drl::pop::Plan& p = holder[0];
    ActPlan& A = aholder[0];
    int bad = 0;
    if (const char* msg = drl::pop::plan(&d, 1, 1, &p)) {
        printf("refused: %s\n", msg);
        return 1;
    }
    if (const char* msg = act_plan(p, &A)) {
        printf("no act plan: %s\n", msg);
        return 1;
    }
    const drl::ll::Plan& P = p.P;
    const int L = P.n_layers;
    EXPECT(A.lds_bytes == 4 * (A.a_floats + A.b_floats + A.w_floats) && A.lds_bytes <= kLdsLimit);
    EXPECT(A.a_floats % 4 == 0 && A.b_floats % 4 == 0 && A.w_floats == kPassUnits * kChunkK);
    EXPECT(stride_ok(A.ldx) && stride_ok(A.lda));
    EXPECT(kEnvTile * code_row_words(P.code_w) <= A.w_floats);  // (the tile's raw code rows fit the staging area)
    EXPECT(code_row_words(P.code_w) * 2 >= P.code_w * P.code_w);
    EXPECT(A.ldx >= P.in4 && P.in4 >= P.in[0] && P.in4 % 4 == 0);
    // layer l reads region l & 1 (A first) and writes the other
    for (int l = 0; l < L; ++l) {
        const int in_floats = (l & 1) ? A.b_floats : A.a_floats, out_floats = (l & 1) ? A.a_floats : A.b_floats;
        const int ldi = l == 0 ? A.ldx : A.lda;
        EXPECT(kEnvTile * ldi <= in_floats && kEnvTile * A.lda <= out_floats);
        EXPECT(r8(P.out[l]) <= A.lda);  // (a 4-unit store that starts below out[l] ends below r8(out[l]))
        EXPECT((P.in[l] + 3) / 4 * 4 <= ldi);
        if (!count) continue;
        // units: every one once
        std::vector<int> unit((size_t)P.out[l], 0);
        for (int ps = 0; ps < pass_count(P.out[l]); ++ps)
            for (int w = 0; w < kActThreads / 64; ++w)
                for (int h = 0; h < 2; ++h)
                    for (int u = 0; u < kUnitsPerLane; ++u) {
                        const int j = ps * kPassUnits + lane_unit(w, h) + u;
                        if (j < P.out[l]) ++unit[(size_t)j];
                    }
        for (int j = 0; j < P.out[l]; ++j) EXPECT(unit[(size_t)j] == 1);
        // inputs: every one once, nothing past the row's zero pad
        std::vector<int> col((size_t)ldi, 0);
        for (int c = 0; c < chunk_count(P.in[l]); ++c) {
            EXPECT(chunk_quads(P.in[l], c) >= 2 && chunk_quads(P.in[l], c) * 4 <= kChunkK && chunk_quads(P.in[l], c) % 2 == 0);
            for (int q = 0; q < chunk_quads(P.in[l], c); ++q)
                for (int i = 0; i < 4; ++i) {
                    const int k = c * kChunkK + 4 * q + i;
                    if (k >= ldi) {
                        ++bad;
                        printf("  layer %d: column %d past the row\n", l, k);
                    } else {
                        ++col[(size_t)k];
                    }
                }
        }
        for (int k = 0; k < ldi; ++k) EXPECT(col[(size_t)k] == (k < (P.in[l] + 3) / 4 * 4 ? 1 : 0));
    }
    // the staging map: every word of the chunk once (the same for every descriptor: w_floats is checked above)
    std::vector<int> word(count ? (size_t)A.w_floats : 0, 0);
    for (int t = 0; count && t < kActThreads; ++t)
        for (int i = 0; i < kStageLoads; ++i) {
            const int at = stage_unit(t, i) * kChunkK + stage_k(t);
            if (at < 0 || at >= A.w_floats) {
                ++bad;
                printf("  staged word %d outside the chunk\n", at);
            } else {
                ++word[(size_t)at];
            }
        }
    for (int i = 0; count && i < A.w_floats; ++i) EXPECT(word[(size_t)i] == 1);
    if (print)
        printf("PLAN %d %d %d %d %d : %d %d %d %d\n", d.in_features, d.hidden[0], d.hidden[1], d.hidden[2], d.n_actions,
               kEnvTile, A.ldx, A.lda, A.lds_bytes);
    return bad;
}

int main() {
    int bad = 0;
    long n = 0;
    int worst = 0;
    for (int W = 5; W <= 9; W += 2)
        for (int nh = 1; nh <= 3; ++nh) {
            int h[3] = {0, 0, 0};
            for (h[0] = 8; h[0] <= DRL_WIDENET_MAX_WIDTH; h[0] += 8)
                for (h[1] = nh > 1 ? 8 : 0; h[1] <= (nh > 1 ? DRL_WIDENET_MAX_WIDTH : 0); h[1] += 8)
                    for (h[2] = nh > 2 ? 8 : 0; h[2] <= (nh > 2 ? DRL_WIDENET_MAX_WIDTH : 0); h[2] += 8)
                        for (int a = 1; a <= 8; ++a) {
                            const drl_widenet_desc d = desc(W * W * 6, h, nh, a);
                            // (the counting checks where a new layer shape can appear; the rest everywhere)
                            const bool count = nh < 3 || (a == 5 && h[2] % 64 == 0 && h[1] % 32 == 0);
                            bad += check(d, false, count);
                            {
                                drl::pop::Plan p;
                                ActPlan A;
                                if (!drl::pop::plan(&d, 1, 1, &p) && !act_plan(p, &A)) worst = A.lds_bytes > worst ? A.lds_bytes : worst;
                            }
                            ++n;
                            if (bad > 20) {
                                printf("FAILED (%d)\n", bad);
                                return 1;
                            }
                        }
        }
    printf("descriptors %ld, the largest LDS plan %d of %d bytes\n", n, worst, kLdsLimit);
    const int nets[][5] = {{294, 128, 64, 0, 5}, {294, 256, 128, 64, 5}, {294, 16, 16, 0, 5}, {150, 64, 0, 0, 3},
                           {486, 256, 256, 256, 8}, {294, 136, 8, 0, 5}};
    for (const auto& v : nets) {
        const int nh = v[3] ? 3 : v[2] ? 2 : 1;
        bad += check(desc(v[0], &v[1], nh, v[4]), true);
    }
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
