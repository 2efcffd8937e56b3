// CPU check of the large-batch DQN learner's agent block (dronerl_amd/csrc/largelearn/dronerl_largelearn_layout.h,
// the header the kernels and the host API share).  For the train_jax.py nets, odd ones and the widest net the
// description admits (512-128-128-128-8), at batches 1, 65 and 4096 (and some between):
//   * the four parameter sets, the counters and the scratch tile [0, bytes) without overlap, 16-byte aligned, and
//     the parameter offsets follow drl_dqn_layout_query's rule (each tensor padded to 4 floats);
//   * every scratch word of every (row, layer, element) -- both nets' decoded inputs with their pad columns, the
//     rows' action, reward and done, both nets' activations, the deltas with the Q head's pad columns, the squared
//     errors -- lies inside the scratch and no two of them share a word; every region starts on a 16-byte
//     boundary and every row stride is a multiple of 4 words (the kernels' 16-byte loads);
//   * the 16-byte reads the tile loop and the update kernel issue (a whole 4-word group at the end of a row) stay
//     inside the region they read;
//   * the launches' grids cover every row and every unit, and the update kernel's tiles every parameter exactly
//     once (its column in[l] is the bias).
// Batches 0 and 4097 and layer sizes outside the limits must be refused by name.  Stand-alone host code (no HIP),
// built and run by tests/test_large_batch_learner.py under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/largelearn/dronerl_largelearn_layout.h"

using drl::ll::Plan;

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("  line %d: %s\n", __LINE__, #cond);           \
            ++bad;                                                \
        }                                                         \
    } while (0)

struct Net {
    const char* name;
    std::vector<int32_t> sizes;  // in, hidden..., actions
    int code_w;
};

static const char* make(const Net& n, int batch, Plan* P) {
    const int L = (int)n.sizes.size() - 1;
    return drl::ll::plan(L, n.sizes.data(), n.sizes.data() + 1, n.code_w, batch, P);
}

static int check(const Net& n, int batch) {
    // (heap: the sanitizer sees an access past the plan)
    std::vector<Plan> holder(1);
    Plan& P = holder[0];
    int bad = 0;
    if (const char* msg = make(n, batch, &P)) {
        printf("%s: refused: %s\n", n.name, msg);
        return 1;
    }
    const int L = (int)n.sizes.size() - 1;
    const drl_dqn_layout& u = P.pub;
    EXPECT(P.n_layers == L && P.batch == batch && P.code_w == n.code_w);
    // the block: drl_dqn_layout_query's parameter offsets
    int64_t f = 0;
    for (int l = 0; l < L; ++l) {
        EXPECT(P.in[l] == n.sizes[l] && P.out[l] == n.sizes[l + 1]);
        EXPECT(u.weight_off[l] == f && P.woff[l] == f);
        f += ((int64_t)P.in[l] * P.out[l] + 3) / 4 * 4;
        EXPECT(u.bias_off[l] == f && P.boff[l] == f);
        f += (P.out[l] + 3) / 4 * 4;
        EXPECT(P.ld[l] % 4 == 0 && P.ld[l] >= P.out[l] && P.ld[l] < P.out[l] + 4);
    }
    EXPECT(u.n_params == f && P.n_params == f);
    EXPECT(P.in4 % 4 == 0 && P.in4 >= P.in[0] && P.in4 < P.in[0] + 4);
    const int64_t offs[7] = {u.online_off, u.target_off, u.m_off, u.v_off, u.counters_off, u.scratch_off, u.bytes};
    const int64_t need[6] = {f * 4, f * 4, f * 4, f * 4, 64, P.scratch_words * 4};
    EXPECT(offs[0] == 0);
    for (int i = 0; i < 6; ++i) {
        EXPECT(offs[i] % 16 == 0);
        EXPECT(offs[i] + need[i] <= offs[i + 1]);
    }
    EXPECT(u.grad_workgroups == 0 && u.grad_lds_bytes == 0);
    // the scratch
    std::vector<char> word((size_t)P.scratch_words, 0);
    auto take = [&](int64_t w) {
        if (w < 0 || w >= P.scratch_words || word[(size_t)w]) {
            if (bad < 8) EXPECT(!"a scratch word outside the scratch, or used twice");
            else ++bad;
            return;
        }
        word[(size_t)w] = 1;
    };
    const int64_t starts[] = {P.x_off[0], P.x_off[1], P.act_off, P.rew_off, P.done_off, P.sq_off};
    for (int64_t s : starts) EXPECT(s % 4 == 0);
    for (int b = 0; b < batch; ++b) {
        for (int net = 0; net < 2; ++net) {
            for (int k = 0; k < P.in4; ++k) take(drl::ll::x_word(P, net, b, k));  // (the pad columns are written)
            for (int l = 0; l < L; ++l)
                for (int j = 0; j < P.out[l]; ++j) take(drl::ll::h_word(P, net, l, b, j));
        }
        for (int l = 0; l < L; ++l) {
            const int cols = l + 1 == L ? P.ld[l] : P.out[l];  // (the TD kernel zeroes the Q head's pad columns)
            for (int j = 0; j < cols; ++j) take(drl::ll::d_word(P, l, b, j));
        }
        take(P.act_off + b);
        take(P.rew_off + b);
        take(P.done_off + b);
        take(P.sq_off + b);
    }
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < L; ++l) EXPECT(P.h_off[net][l] % 4 == 0 && P.d_off[l] % 4 == 0);
    // the 16-byte reads: the last 4-word group of the last row of every operand the tile loop and the update read
    auto group_in = [&](int64_t region, int64_t lda, int K) {  // words [g, g + 4) of row batch - 1
        const int64_t g = region + (int64_t)(batch - 1) * lda + (K + 3) / 4 * 4 - 4;
        return g >= 0 && g + 4 <= P.scratch_words && lda % 4 == 0 && lda >= (K + 3) / 4 * 4;
    };
    for (int net = 0; net < 2; ++net) {
        EXPECT(group_in(P.x_off[net], P.in4, P.in[0]));
        for (int l = 1; l < L; ++l) EXPECT(group_in(P.h_off[net][l - 1], P.ld[l - 1], P.in[l]));
    }
    for (int l = 0; l < L; ++l) EXPECT(group_in(P.d_off[l], P.ld[l], P.out[l]));
    // the grids: row tiles x unit tiles cover every (row, unit) once; the update items every parameter once
    EXPECT(drl::ll::row_tiles(P) * drl::ll::kTileRows >= batch && (drl::ll::row_tiles(P) - 1) * drl::ll::kTileRows < batch);
    for (int l = 0; l < L; ++l) {
        const int t = drl::ll::unit_tiles(P.out[l]);
        EXPECT(t * drl::ll::kTileUnits >= P.out[l] && (t - 1) * drl::ll::kTileUnits < P.out[l]);
        std::vector<char> hit((size_t)f, 0);
        const int kt = drl::ll::update_col_tiles(P, l), jt = drl::ll::update_unit_tiles(P, l);
        EXPECT((kt - 1) * drl::ll::kUpdateCols <= P.in[l] && kt * drl::ll::kUpdateCols > P.in[l]);  // (column in[l]: the bias)
        EXPECT((jt - 1) * drl::ll::kUpdateUnits < P.out[l] && jt * drl::ll::kUpdateUnits >= P.out[l]);
        for (int k = 0; k < kt * drl::ll::kUpdateCols && !bad; ++k)  // (every thread's four entries, as the kernel)
            for (int j = 0; j < jt * drl::ll::kUpdateUnits; ++j) {
                const int64_t i = drl::ll::update_param(P, l, j, k);
                if (i < 0) {
                    EXPECT(j >= P.out[l] || k > P.in[l]);
                    continue;
                }
                EXPECT(i < f && (k == P.in[l] ? i >= P.boff[l] && i < P.boff[l] + P.out[l]
                                              : i >= P.woff[l] && i < P.boff[l]) && !hit[(size_t)i]);
                if (i < f) hit[(size_t)i] = 1;
            }
        int64_t hits = 0;
        for (char c : hit) hits += c;
        EXPECT(hits == (int64_t)P.in[l] * P.out[l] + P.out[l]);
    }
    printf("%s (batch %d): n_params %lld, scratch %lld words, block %lld B: %s\n", n.name, batch, (long long)f,
           (long long)P.scratch_words, (long long)u.bytes, bad ? "FAILED" : "ok");
    return bad;
}

static int refused(const char* name, const Net& n, int batch, const char* word) {
    std::vector<Plan> holder(1);
    const char* msg = make(n, batch, &holder[0]);
    if (!msg || !strstr(msg, word)) {
        printf("%s: expected a refusal naming '%s', got: %s\n", name, word, msg ? msg : "(accepted)");
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    const Net c3{"294-128-64-5 code", {294, 128, 64, 5}, 7};
    const Net narrow{"294-16-16-5 code", {294, 16, 16, 5}, 7};
    const Net three{"294-96-32-32-5", {294, 96, 32, 32, 5}, 7};
    const Net r2{"150-64-5", {150, 64, 5}, 0};
    const Net widest{"512-128-128-128-8", {512, 128, 128, 128, 8}, 0};
    const Net tiny{"4-8-1", {4, 8, 1}, 0};
    const Net three_actions{"30-24-3", {30, 24, 3}, 0};
    for (int batch : {1, 65, 4096}) {
        bad += check(c3, batch);
        bad += check(widest, batch);
    }
    bad += check(narrow, 1000);
    bad += check(three, 96);
    bad += check(r2, 130);
    bad += check(c3, 257);
    bad += check(tiny, 64);
    bad += check(three_actions, 200);
    bad += refused("batch 0", c3, 0, "batch");
    bad += refused("batch 4097", c3, 4097, "batch");
    bad += refused("one layer", Net{"x", {294, 5}, 0}, 8, "n_hidden");
    bad += refused("wide hidden", Net{"x", {294, 136, 5}, 0}, 8, "limits");
    bad += refused("nine actions", Net{"x", {294, 64, 9}, 0}, 8, "limits");
    bad += refused("wide input", Net{"x", {516, 64, 5}, 0}, 8, "limits");
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
