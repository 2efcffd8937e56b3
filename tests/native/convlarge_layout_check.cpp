// CPU check of the large-batch conv DQN learner's agent block
// (dronerl_amd/csrc/convlarge/dronerl_convlarge_layout.h, the header the kernels and the host API share).  For
// every net of tests/test_conv_large_batch_learner.py's table (a-i and the sweep net s) and for the corners of
// the limits, at batches on both sides of a chunk boundary and at the limit:
//   * the four parameter sets, the counters and the scratch tile [0, bytes) without overlap, 16-byte aligned;
//     the parameter sets and a row's words are the conv learner's own plan;
//   * every scratch word -- the rows' squared errors, every (row, layer, element) of the rows' inputs,
//     activations and deltas, every (chunk, parameter) partial gradient -- lies inside the scratch and no two of
//     them share a word;
//   * the dense partials' tiles: over a chunk's tiles every dense weight and bias is taken by exactly one
//     (tile, column, unit), and no tile reaches outside its layer's [W | b];
//   * the conv partials' groups: every conv weight and bias is taken by exactly one (group, ky, kx);
//   * chunks == ceil(batch / 64) and every chunk has between 1 and 64 rows.
// A batch outside [1, 4096] and a net whose per-row working set is too large must be refused by name.
// Stand-alone host code (no HIP), built and run by tests/test_conv_large_batch_learner.py under the address and
// undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/convlarge/dronerl_convlarge_layout.h"

using drl::cg::Plan;
using drl::cg::TileRef;
using drl::cl::LLayer;

struct ConvSpec {
    int co, k, s, p;
};

static drl_convnet_desc make(int W, std::vector<ConvSpec> conv, std::vector<int> dense, int actions = 5,
                             int input = DRL_QNET_INPUT_OBS) {
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

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("  line %d: %s\n", __LINE__, #cond);           \
            ++bad;                                                \
        }                                                         \
    } while (0)

static int check(const char* name, const drl_convnet_desc& d, int batch) {
    // (heap: the sanitizer sees an access past the plan)
    std::vector<Plan> holder(1);
    std::vector<drl::cl::Plan> small(1);
    Plan& P = holder[0];
    int bad = 0;
    if (const char* msg = drl::cg::plan(&d, batch, &P)) {
        printf("%s: refused: %s\n", name, msg);
        return 1;
    }
    if (drl::cl::plan(&d, 1, &small[0])) {
        printf("%s: the conv learner's plan refuses the net\n", name);
        return 1;
    }
    const drl::cl::Plan& C = P.c;
    const drl::cg::Tiles& T = P.t;
    const drl_convnet_dqn_layout& u = C.pub;
    // the conv learner's parameter sets and row
    const drl::cl::Plan& S = small[0];
    EXPECT(C.n_params == S.n_params && C.row_words == S.row_words && C.n_layers == S.n_layers && C.in == S.in);
    EXPECT(u.online_off == S.pub.online_off && u.target_off == S.pub.target_off && u.m_off == S.pub.m_off &&
           u.v_off == S.pub.v_off && u.counters_off == S.pub.counters_off && u.scratch_off == S.pub.scratch_off);
    for (int l = 0; l < C.n_layers; ++l) {
        EXPECT(C.l[l].woff == S.l[l].woff && C.l[l].boff == S.l[l].boff && C.l[l].in == S.l[l].in &&
               C.l[l].act == S.l[l].act && C.l[l].delta == S.l[l].delta);
        EXPECT(u.weight_off[l] == C.l[l].woff && u.bias_off[l] == C.l[l].boff);
    }
    const int64_t sum = C.n_params;
    const int64_t offs[7] = {u.online_off, u.target_off, u.m_off, u.v_off, u.counters_off, u.scratch_off, u.bytes};
    const int64_t need[6] = {sum * 4, sum * 4, sum * 4, sum * 4, 64, C.scratch_words * 4};
    EXPECT(offs[0] == 0);
    for (int i = 0; i < 6; ++i) {
        EXPECT(offs[i] % 16 == 0);
        EXPECT(offs[i] + need[i] <= offs[i + 1]);
    }
    EXPECT(C.batch == batch && u.row_bytes == C.row_words * 4 && u.row_bytes <= drl::cl::kRowLdsMax);
    // the chunks
    EXPECT(T.chunks == (batch + 63) / 64 && T.chunks >= 1 && T.chunks <= drl::cg::kMaxChunks);
    EXPECT((T.chunks - 1) * drl::cg::kChunkRows < batch && batch <= T.chunks * drl::cg::kChunkRows);
    // the scratch
    std::vector<char> word((size_t)C.scratch_words, 0);
    auto take = [&](int64_t w) {
        if (w < 0 || w >= C.scratch_words || word[(size_t)w]) {
            if (bad < 8) EXPECT(!"a scratch word outside the scratch, or used twice");
            else ++bad;
            return;
        }
        word[(size_t)w] = 1;
    };
    for (int b = 0; b < drl::cg::kMaxBatch; ++b) take(C.sq_off + b);
    for (int b = 0; b < batch && bad < 8; ++b) {
        for (int e = 0; e < C.in; ++e) take(drl::cl::row_word(C, b, -1, 0, e));
        for (int l = 0; l < C.n_layers; ++l) {
            const LLayer& q = C.l[l];
            if (q.act >= 0)
                for (int e = 0; e < q.n_out; ++e) take(drl::cl::row_word(C, b, l, 0, e));
            for (int e = 0; e < q.n_out; ++e) take(drl::cl::row_word(C, b, l, 1, e));
        }
    }
    for (int c = 0; c < T.chunks && bad < 8; ++c)
        for (int64_t i = 0; i < sum; ++i) take(drl::cg::part_word(C, T, c, i));
    // the dense partials' tiles
    std::vector<char> hit((size_t)sum, 0);
    const int64_t nconv = C.l[C.n_conv].woff;
    EXPECT(T.dense_tiles == T.tile_base[C.n_layers] && T.dense_tiles >= 1);
    for (int t = 0; t < T.dense_tiles && bad < 8; ++t) {
        const TileRef r = drl::cg::tile_locate(C, T, t);
        EXPECT(r.layer >= C.n_conv && r.layer < C.n_layers);
        if (r.layer < C.n_conv || r.layer >= C.n_layers) break;
        const LLayer& q = C.l[r.layer];
        EXPECT(!q.conv && t >= T.tile_base[r.layer] && t < T.tile_base[r.layer + 1]);
        EXPECT(r.k0 >= 0 && r.k0 <= q.K && r.k0 % drl::cg::kTileCols == 0);
        EXPECT(r.j0 >= 0 && r.j0 < q.n_out && r.j0 % drl::cg::kTileUnits == 0);
        for (int k = r.k0; k < r.k0 + drl::cg::kTileCols && k <= q.K; ++k)      // (the kernel's own store bounds)
            for (int j = r.j0; j < r.j0 + drl::cg::kTileUnits && j < q.n_out; ++j) {
                const int64_t i = k < q.K ? q.woff + (int64_t)j * q.K + k : q.boff + j;
                if (i < nconv || i >= sum || hit[(size_t)i]) {
                    EXPECT(!"a dense parameter outside the dense layers, or taken by two tiles");
                    continue;
                }
                hit[(size_t)i] = 1;
            }
    }
    for (int64_t i = 0; i < sum; ++i)
        if (hit[(size_t)i] != (i >= nconv)) {
            EXPECT(!"a dense parameter no tile takes, or a conv parameter a tile takes");
            break;
        }
    // the conv partials' groups: every conv parameter in exactly one (group, ky, kx), or one bias group
    std::vector<char> chit((size_t)sum, 0);
    EXPECT(T.conv_groups == T.group_base[C.n_conv] && T.conv_groups >= 1);
    for (int g = 0; g < T.conv_groups && bad < 8; ++g) {
        const drl::cg::GroupRef r = drl::cg::group_locate(C, T, g);
        EXPECT(r.layer >= 0 && r.layer < C.n_conv);
        if (r.layer < 0 || r.layer >= C.n_conv) break;
        const LLayer& q = C.l[r.layer];
        EXPECT(q.conv && q.k >= 1 && q.k <= drl::cg::kMaxKernel && r.co >= 0 && r.co < q.cout && r.ci >= 0 &&
               r.ci <= q.cin);
        EXPECT(g >= T.group_base[r.layer] && g < T.group_base[r.layer + 1]);
        for (int e = 0; e < (r.ci == q.cin ? 1 : q.k * q.k); ++e) {
            // (the kernel's own store addresses)
            const int64_t i = r.ci == q.cin ? q.boff + r.co : q.woff + ((int64_t)r.co * q.cin + r.ci) * (q.k * q.k) + e;
            if (r.ci < q.cin)
                EXPECT(i == drl::cl::param_index(C, drl::cl::ParamRef{r.layer, 0, r.co, r.ci, e / q.k, e % q.k}));
            if (i < 0 || i >= nconv || chit[(size_t)i]) {
                EXPECT(!"a conv parameter outside the conv layers, or taken by two groups");
                continue;
            }
            chit[(size_t)i] = 1;
        }
    }
    for (int64_t i = 0; i < sum; ++i)
        if (chit[(size_t)i] != (i < nconv)) {
            EXPECT(!"a conv parameter no group takes, or a dense parameter a group takes");
            break;
        }
    EXPECT(T.rows_threads >= 256 && T.rows_threads <= drl::cg::kRowsThreadsMax && T.rows_threads % 256 == 0);
    printf("%s (batch %d): n_params %lld, row %d B, %d chunks, %d dense tiles, block %lld B: %s\n", name, batch,
           (long long)sum, u.row_bytes, T.chunks, T.dense_tiles, (long long)u.bytes, bad ? "FAILED" : "ok");
    return bad;
}

static int refused(const char* name, const drl_convnet_desc* d, int batch, const char* word) {
    std::vector<Plan> holder(1);
    const char* msg = drl::cg::plan(d, batch, &holder[0]);
    if (!msg || !strstr(msg, word)) {
        printf("%s: expected a refusal naming '%s', got: %s\n", name, word, msg ? msg : "(accepted)");
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    struct Net {
        const char* name;
        drl_convnet_desc d;
    };
    const Net nets[] = {
        {"a", make(7, {{4, 3, 1, 1}}, {8})},
        {"b", make(7, {{8, 3, 1, 1}}, {}, 5, DRL_QNET_INPUT_CODE)},
        {"c", make(9, {{8, 3, 1, 0}, {12, 3, 2, 1}}, {16, 8}, 5, DRL_QNET_INPUT_CODE)},
        {"e", make(3, {{32, 1, 1, 0}}, {8})},
        {"f", make(7, {{6, 2, 3, 0}}, {})},
        {"g", make(5, {{5, 5, 1, 2}}, {128}, 5, DRL_QNET_INPUT_CODE)},
        {"h", make(9, {{8, 3, 1, 1}, {8, 3, 2, 0}, {16, 2, 1, 0}}, {}, 5, DRL_QNET_INPUT_CODE)},
        {"i", make(7, {{5, 3, 1, 1}, {7, 2, 3, 0}}, {8})},
        {"s", make(7, {{16, 3, 1, 1}, {32, 3, 1, 1}}, {128, 64}, 5, DRL_QNET_INPUT_CODE)},
    };
    const int batches[] = {1, 64, 65, 1000, 4096};
    for (const Net& n : nets)
        for (int batch : batches) bad += check(n.name, n.d, batch);
    // the limits' corners: the smallest net, one action, the widest accepted row at the largest batch
    bad += check("smallest", make(3, {{1, 1, 3, 0}}, {}, 1), 4096);
    bad += check("eight actions", make(5, {{3, 5, 1, 0}}, {8, 128}, 8), 4095);
    bad += check("widest row", make(9, {{32, 3, 1, 1}, {32, 3, 1, 1}, {32, 3, 1, 1}}, {}, 8), 4096);
    const drl_convnet_desc big = make(9, {{32, 1, 1, 4}}, {});  // a 17 x 17 x 32 map: 2 x 36,992 B of a row
    bad += refused("row too large", &big, 256, "DRL_CONVNET_DQN_ROW_BYTES_MAX");
    bad += refused("batch 0", &nets[0].d, 0, "batch");
    bad += refused("batch 4097", &nets[0].d, 4097, "batch");
    bad += refused("NULL desc", nullptr, 256, "NULL");
    const drl_convnet_desc even = make(6, {{4, 3, 1, 1}}, {});
    bad += refused("even window", &even, 256, "window");
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
