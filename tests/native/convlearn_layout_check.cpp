// CPU check of the conv DQN learner's agent block (dronerl_amd/csrc/convlearn/dronerl_convlearn_layout.h, the
// header the kernels and the host API share).  For every net of tests/_conv_learner_ref.py's table and for the
// corners of the limits:
//   * the four parameter sets, the counters and the scratch tile [0, bytes) without overlap, 16-byte aligned, and
//     n_params is the sum of every layer's weights and biases;
//   * the parameter index <-> (layer, bias, co, ci, ky, kx) map of the update kernel is a bijection onto
//     [0, n_params), with every field inside its layer's bounds;
//   * every scratch word of every (row, layer, element) -- the row's input, each layer's activations and deltas,
//     the rows' squared errors -- lies inside the scratch and no two of them share a word; each layer reads its
//     input where the previous one wrote its activations; a row fits the rows kernel's LDS.
// A batch outside [1, 64] and a net whose per-row working set is too large must be refused by name.  Stand-alone
// host code (no HIP), built and run by tests/test_convnet_learner.py under the address and undefined-behaviour
// sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/convlearn/dronerl_convlearn_layout.h"

using drl::cl::LLayer;
using drl::cl::ParamRef;
using drl::cl::Plan;

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
    Plan& P = holder[0];
    int bad = 0;
    if (const char* msg = drl::cl::plan(&d, batch, &P)) {
        printf("%s: refused: %s\n", name, msg);
        return 1;
    }
    const drl_convnet_dqn_layout& u = P.pub;
    // the block
    int64_t sum = 0;
    for (int l = 0; l < P.n_layers; ++l) {
        const LLayer& q = P.l[l];
        EXPECT(u.weight_off[l] == sum && q.woff == sum);
        sum += (int64_t)q.cout * q.K;
        EXPECT(u.bias_off[l] == sum && q.boff == sum);
        sum += q.cout;
        EXPECT(q.K == (q.conv ? q.cin * q.k * q.k : q.n_in));
        EXPECT(l == 0 ? q.n_in == P.in : q.n_in == P.l[l - 1].n_out);
        EXPECT(q.in == (l == 0 ? 0 : P.l[l - 1].act));
        EXPECT((q.act < 0) == (l + 1 == P.n_layers));
    }
    EXPECT(u.n_params == sum && P.n_params == sum && u.n_layers == P.n_layers);
    const int64_t offs[7] = {u.online_off, u.target_off, u.m_off, u.v_off, u.counters_off, u.scratch_off, u.bytes};
    const int64_t need[6] = {sum * 4, sum * 4, sum * 4, sum * 4, 64, P.scratch_words * 4};
    EXPECT(offs[0] == 0);
    for (int i = 0; i < 6; ++i) {
        EXPECT(offs[i] % 16 == 0);
        EXPECT(offs[i] + need[i] <= offs[i + 1]);
    }
    EXPECT(u.row_bytes == P.row_words * 4 && u.row_bytes <= drl::cl::kRowLdsMax && P.row_words % 4 == 0);
    // the parameter map
    std::vector<char> hit((size_t)sum, 0);
    for (int64_t i = 0; i < sum; ++i) {
        const ParamRef r = drl::cl::param_locate(P, i);
        EXPECT(r.layer >= 0 && r.layer < P.n_layers);
        if (r.layer < 0 || r.layer >= P.n_layers) break;
        const LLayer& q = P.l[r.layer];
        EXPECT(r.co >= 0 && r.co < q.cout);
        if (!r.bias) EXPECT(r.ci >= 0 && r.ci < q.cin && r.ky >= 0 && r.ky < q.k && r.kx >= 0 && r.kx < q.k);
        EXPECT(drl::cl::param_index(P, r) == i);
        if (bad) break;
    }
    for (int l = 0; l < P.n_layers && !bad; ++l) {
        const LLayer& q = P.l[l];
        for (int co = 0; co < q.cout; ++co) {
            const int64_t bi = drl::cl::param_index(P, ParamRef{l, 1, co, 0, 0, 0});
            EXPECT(bi >= 0 && bi < sum && !hit[(size_t)bi]);
            if (bi >= 0 && bi < sum) hit[(size_t)bi] = 1;
            for (int ci = 0; ci < q.cin; ++ci)
                for (int ky = 0; ky < q.k; ++ky)
                    for (int kx = 0; kx < q.k; ++kx) {
                        const int64_t wi = drl::cl::param_index(P, ParamRef{l, 0, co, ci, ky, kx});
                        if (wi < 0 || wi >= sum || hit[(size_t)wi]) {
                            EXPECT(!"a weight outside the set, or hit twice");
                            continue;
                        }
                        hit[(size_t)wi] = 1;
                    }
        }
    }
    for (int64_t i = 0; i < sum; ++i)
        if (!hit[(size_t)i]) {
            EXPECT(!"a parameter no tensor element maps to");
            break;
        }
    // the scratch
    std::vector<char> word((size_t)P.scratch_words, 0);
    auto take = [&](int64_t w) {
        if (w < 0 || w >= P.scratch_words || word[(size_t)w]) {
            EXPECT(!"a scratch word outside the scratch, or used twice");
            return;
        }
        word[(size_t)w] = 1;
    };
    for (int b = 0; b < drl::cl::kMaxBatch; ++b) take(P.sq_off + b);
    for (int b = 0; b < batch && bad < 8; ++b) {
        for (int e = 0; e < P.in; ++e) take(drl::cl::row_word(P, b, -1, 0, e));
        for (int l = 0; l < P.n_layers; ++l) {
            const LLayer& q = P.l[l];
            if (q.act >= 0)
                for (int e = 0; e < q.n_out; ++e) take(drl::cl::row_word(P, b, l, 0, e));
            for (int e = 0; e < q.n_out; ++e) take(drl::cl::row_word(P, b, l, 1, e));
            EXPECT(q.delta + q.n_out <= P.row_words && (q.act < 0 || q.act + q.n_out <= P.row_words));
        }
    }
    printf("%s (batch %d): n_params %lld, row %d B, block %lld B: %s\n", name, batch, (long long)sum, u.row_bytes,
           (long long)u.bytes, bad ? "FAILED" : "ok");
    return bad;
}

static int refused(const char* name, const drl_convnet_desc* d, int batch, const char* word) {
    std::vector<Plan> holder(1);
    const char* msg = drl::cl::plan(d, batch, &holder[0]);
    if (!msg || !strstr(msg, word)) {
        printf("%s: expected a refusal naming '%s', got: %s\n", name, word, msg ? msg : "(accepted)");
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    const drl_convnet_desc a = make(7, {{4, 3, 1, 1}}, {8});
    const drl_convnet_desc b = make(7, {{8, 3, 1, 1}}, {}, 5, DRL_QNET_INPUT_CODE);
    const drl_convnet_desc c = make(9, {{8, 3, 1, 0}, {12, 3, 2, 1}}, {16, 8}, 5, DRL_QNET_INPUT_CODE);
    const drl_convnet_desc e = make(3, {{32, 1, 1, 0}}, {8});
    const drl_convnet_desc f = make(7, {{6, 2, 3, 0}}, {});
    const drl_convnet_desc g = make(5, {{5, 5, 1, 2}}, {128}, 5, DRL_QNET_INPUT_CODE);
    const drl_convnet_desc h = make(9, {{8, 3, 1, 1}, {8, 3, 2, 0}, {16, 2, 1, 0}}, {}, 5, DRL_QNET_INPUT_CODE);
    const drl_convnet_desc i = make(7, {{5, 3, 1, 1}, {7, 2, 3, 0}}, {8});
    bad += check("a", a, 1);
    bad += check("b", b, 8);
    bad += check("c", c, 5);
    bad += check("e", e, 8);
    bad += check("f", f, 64);
    bad += check("g", g, 16);
    bad += check("h", h, 8);
    bad += check("i", i, 8);
    // the limits' corners: the smallest net, one action, the widest accepted row at the largest batch
    bad += check("smallest", make(3, {{1, 1, 3, 0}}, {}, 1), 1);
    bad += check("eight actions", make(5, {{3, 5, 1, 0}}, {8, 128}, 8), 64);
    bad += check("widest row", make(9, {{32, 3, 1, 1}, {32, 3, 1, 1}, {32, 3, 1, 1}}, {}, 8), 64);
    const drl_convnet_desc big = make(9, {{32, 1, 1, 4}}, {});  // a 17 x 17 x 32 map: 2 x 36,992 B of a row
    bad += refused("row too large", &big, 8, "DRL_CONVNET_DQN_ROW_BYTES_MAX");
    bad += refused("batch 0", &a, 0, "batch");
    bad += refused("batch 65", &a, 65, "batch");
    bad += refused("NULL desc", nullptr, 8, "NULL");
    const drl_convnet_desc even = make(6, {{4, 3, 1, 1}}, {});
    bad += refused("even window", &even, 8, "window");
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
