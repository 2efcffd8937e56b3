// CPU check of the population's block (dronerl_amd/csrc/population/dronerl_population_layout.h, the header the
// kernels and the host API share).  For the sweep's nets at several population sizes and batches:
//   * a member block's offsets equal the single-agent plan's (drl::ll::plan with the wide width limit, which is
//     what drl_dqn_large_layout_query / drl_widenet_dqn_layout_query report), so a member's slice can be handed
//     to the single-agent code;
//   * the member blocks and the hyperparameter records tile [0, bytes) without overlap; the stride and every
//     member's start keep 16-byte alignment, every record 8-byte alignment and its own kHRecStride bytes;
//   * every scratch word of every member (both nets' inputs, action, reward, done, activations, deltas, squared
//     errors, for every row below max_batch) is placed once over the whole population: a byte map of the
//     allocation counts one writer per word;
//   * the act's LDS (the decoded inputs and two activation buffers of kActEnvs rows) holds every layer's row and
//     stays within 64 KB; its row strides are multiples of 4 floats (16-byte LDS reads);
//   * members 0 and 1025, max_batch 0 and 4097, a width of 12 or 264, a window that is not 5, 7 or 9, an f32-row
//     net and NULL are refused by name.
// Stand-alone host code (no HIP), built and run by tests/test_population.py under the address and
// undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/population/dronerl_population_layout.h"

using drl::pop::Plan;

#define EXPECT(cond)                                    \
    do {                                                \
        if (!(cond)) {                                  \
            printf("  line %d: %s\n", __LINE__, #cond); \
            ++bad;                                      \
        }                                               \
    } while (0)

static drl_widenet_desc desc(int in, std::vector<int> hidden, int actions = 5, int input = DRL_QNET_INPUT_CODE) {
    drl_widenet_desc d = {};
    d.in_features = in;
    d.n_hidden = (int)hidden.size();
    for (size_t i = 0; i < hidden.size() && i < 3; ++i) d.hidden[i] = hidden[i];
    d.n_actions = actions;
    d.input = input;
    return d;
}

static int check(const drl_widenet_desc& d, int members, int max_batch) {
    std::vector<Plan> holder(1);  // (heap: the sanitizer sees an access past the plan)
    Plan& p = holder[0];
    int bad = 0;
    if (const char* msg = drl::pop::plan(&d, members, max_batch, &p)) {
        printf("refused: %s\n", msg);
        return 1;
    }
    const drl::ll::Plan& P = p.P;
    // a member block is the single agent's
    const int L = d.n_hidden + 1;
    int32_t in[4], out[4];
    for (int l = 0; l < L; ++l) {
        in[l] = l == 0 ? d.in_features : d.hidden[l - 1];
        out[l] = l + 1 < L ? d.hidden[l] : d.n_actions;
    }
    std::vector<drl::ll::Plan> one(1);
    EXPECT(drl::ll::plan(L, in, out, P.code_w, max_batch, &one[0], DRL_WIDENET_MAX_WIDTH) == nullptr);
    EXPECT(memcmp(&one[0].pub, &P.pub, sizeof P.pub) == 0);
    EXPECT(one[0].scratch_words == P.scratch_words && one[0].n_params == P.n_params);
    EXPECT(P.code_w * P.code_w * 6 == d.in_features);
    // tiling and alignment
    EXPECT(p.stride % 16 == 0 && p.stride >= P.pub.bytes && p.stride < P.pub.bytes + 16);
    EXPECT(p.hp_off == p.stride * members && p.hp_off % 16 == 0);
    EXPECT(p.bytes == p.hp_off + drl::pop::kHRecStride * members);
    EXPECT(drl::pop::kHRecStride >= (int64_t)sizeof(drl::pop::HRec) && drl::pop::kHRecStride % 16 == 0);
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
    for (int m = 0; m < members; ++m) {
        const int64_t b0 = drl::pop::member_off(p, m);
        EXPECT(b0 % 16 == 0);
        const int64_t sets[4] = {P.pub.online_off, P.pub.target_off, P.pub.m_off, P.pub.v_off};
        for (int s = 0; s < 4; ++s) mark(b0 + sets[s], P.n_params * 4);
        EXPECT(P.pub.v_off == P.pub.m_off + P.n_params * 4);  // (the init kernel clears both moment sets as one run)
        mark(b0 + P.pub.counters_off, 64);
        const int64_t s0 = b0 + P.pub.scratch_off;
        // every scratch word of every row, once
        for (int b = 0; b < max_batch; ++b) {
            for (int n = 0; n < 2; ++n) mark(s0 + 4 * drl::ll::x_word(P, n, b, 0), 4 * (int64_t)P.in4);
            mark(s0 + 4 * (P.act_off + b), 4);
            mark(s0 + 4 * (P.rew_off + b), 4);
            mark(s0 + 4 * (P.done_off + b), 4);
            mark(s0 + 4 * (P.sq_off + b), 4);
            for (int l = 0; l < L; ++l) {
                for (int n = 0; n < 2; ++n) mark(s0 + 4 * drl::ll::h_word(P, n, l, b, 0), 4 * (int64_t)P.ld[l]);
                mark(s0 + 4 * drl::ll::d_word(P, l, b, 0), 4 * (int64_t)P.ld[l]);
            }
        }
        const int64_t h0 = drl::pop::hrec_off(p, m);
        EXPECT(h0 % 16 == 0);
        mark(h0, (int64_t)sizeof(drl::pop::HRec));
    }
    // the act's LDS
    EXPECT(p.act_ldx % 4 == 0 && p.act_ldh % 4 == 0 && p.act_ldx >= d.in_features);
    for (int l = 0; l < L; ++l) EXPECT(p.act_ldh >= out[l] && out[l] <= drl::pop::kActThreads);
    EXPECT(p.act_lds_bytes == 4 * drl::pop::kActEnvs * (p.act_ldx + 2 * p.act_ldh) && p.act_lds_bytes <= 65536);
    // the grids' limits (members in blockIdx.y / z)
    EXPECT(2 * members <= 65535 && L * members <= 65535);
    return bad;
}

static int refused(const drl_widenet_desc* d, int members, int max_batch, const char* word) {
    std::vector<Plan> holder(1);
    const char* msg = drl::pop::plan(d, members, max_batch, &holder[0]);
    if (!msg || !strstr(msg, word)) {
        printf("  expected a refusal naming '%s', got: %s\n", word, msg ? msg : "(accepted)");
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    const drl_widenet_desc nets[] = {desc(294, {128, 64}), desc(294, {256, 128, 64}), desc(294, {16, 16}),
                                     desc(150, {64}), desc(486, {256, 256, 256}, 8), desc(294, {136, 8}, 1)};
    for (const drl_widenet_desc& d : nets) {
        bad += check(d, 1, 1);
        bad += check(d, 4, 40);
        bad += check(d, 3, 65);
    }
    bad += check(desc(150, {8}), 1024, 8);
    bad += check(desc(294, {128, 64}), 2, 4096);
    const drl_widenet_desc ok = desc(294, {128, 64});
    bad += refused(&ok, 0, 8, "members");
    bad += refused(&ok, 1025, 8, "members");
    bad += refused(&ok, 4, 0, "max_batch");
    bad += refused(&ok, 4, 4097, "max_batch");
    bad += refused(nullptr, 4, 8, "NULL");
    const drl_widenet_desc w12 = desc(294, {12}), w264 = desc(294, {264}), win = desc(11 * 11 * 6, {64}),
                           win3 = desc(54, {64}), obs = desc(294, {64}, 5, DRL_QNET_INPUT_OBS), a9 = desc(294, {64}, 9),
                           h4 = desc(294, {}), a0 = desc(294, {64}, 0);
    bad += refused(&w12, 4, 8, "hidden widths");
    bad += refused(&w264, 4, 8, "hidden widths");
    bad += refused(&win, 4, 8, "window");
    bad += refused(&win3, 4, 8, "window");
    bad += refused(&obs, 4, 8, "policy code");
    bad += refused(&a9, 4, 8, "n_actions");
    bad += refused(&a0, 4, 8, "n_actions");
    bad += refused(&h4, 4, 8, "n_hidden");
    printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
