// widenet_layout_check.cpp — a stand-alone check of dronerl_amd/csrc/widenet/dronerl_widenet_layout.h (built by
// tests/test_wide_nets.py under the address and undefined-behaviour sanitizers; no device, nothing loaded into
// Python).  For each net: every (layer, unit, input, piece) maps to a distinct in-bounds fp16 element of the
// image and every other fragment element is a pad that frag_elem names as one; the biases and the status vector
// are disjoint from the fragments and each other; every LDS word the act's plan touches (the staging's writes,
// each layer's 16-byte row reads and output stores) lies inside the workgroup's allocation, which is within
// 160 KB, and a layer never writes the region it reads; the learner's plan takes a width-256 net at batches 1,
// 65 and 4096 and still refuses 264 (and 136 at the default limit).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../dronerl_amd/csrc/largelearn/dronerl_largelearn_layout.h"
#include "../../dronerl_amd/csrc/widenet/dronerl_widenet_layout.h"

using namespace drl;

#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            exit(1);                                    \
        }                                               \
    } while (0)

struct Net {
    int in, nh, h[3], actions, input;
};

static void check_net(const Net& n) {
    drl_widenet_desc d{};
    d.in_features = n.in;
    d.n_hidden = n.nh;
    for (int i = 0; i < n.nh; ++i) d.hidden[i] = n.h[i];
    d.n_actions = n.actions;
    d.input = n.input;
    wn::Layout L;
    const char* msg = wn::layout(&d, &L);
    CHECK(!msg, "layout refused %d-%d: %s", n.in, n.h[0], msg ? msg : "");
    CHECK(L.n_layers == n.nh + 1 && L.total_words == L.status + 4 && L.status % 4 == 0, "image marks");
    // ---- the image: 0 = untouched, 1 = weight, 2 = pad, 3 = bias, 4 = bias pad (per fp16 element / per word)
    std::vector<uint8_t> elem((size_t)L.frag_words * 2, 0);
    int64_t weights = 0;
    for (int l = 0; l < L.n_layers; ++l) {
        const wn::Layer& y = L.l[l];
        CHECK(y.kt * 32 >= y.in && y.nt * 16 >= y.out, "layer %d padding", l);
        if (l + 1 < L.n_layers) CHECK(16 * y.nt == 32 * L.l[l + 1].kt, "layer %d's tiles fill layer %d's K-slices", l, l + 1);
        for (int piece = 0; piece < 2; ++piece)
            for (int u = 0; u < y.out; ++u)
                for (int k = 0; k < y.in; ++k) {
                    const int64_t e = wn::weight_elem(y, u, k, piece);
                    CHECK(e >= 0 && e < (int64_t)elem.size(), "layer %d W[%d][%d] piece %d out of the fragments", l, u, k, piece);
                    CHECK(elem[(size_t)e] == 0, "layer %d W[%d][%d] piece %d shares an element", l, u, k, piece);
                    elem[(size_t)e] = 1;
                    ++weights;
                    // the pack kernel's direction names the same weight
                    const int64_t set0 = (int64_t)(piece ? y.frag_lo : y.frag_hi) * 8;
                    int uu, kk;
                    wn::frag_elem(y, e - set0, &uu, &kk);
                    CHECK(uu == u && kk == k, "layer %d frag_elem is not weight_elem's inverse", l);
                }
        // every other element of the layer's two sets is a pad by frag_elem
        for (int piece = 0; piece < 2; ++piece) {
            const int64_t set0 = (int64_t)(piece ? y.frag_lo : y.frag_hi) * 8, n_el = (int64_t)y.nt * y.kt * 512;
            CHECK(set0 + n_el <= (int64_t)elem.size(), "layer %d set %d ends past the fragments", l, piece);
            for (int64_t e = 0; e < n_el; ++e) {
                int uu, kk;
                wn::frag_elem(y, e, &uu, &kk);
                CHECK(uu >= 0 && uu < 16 * y.nt && kk >= 0 && kk < 32 * y.kt, "layer %d element outside the padded GEMM", l);
                if (uu >= y.out || kk >= y.in) {
                    CHECK(elem[(size_t)(set0 + e)] == 0, "layer %d pad element already taken", l);
                    elem[(size_t)(set0 + e)] = 2;
                } else {
                    CHECK(elem[(size_t)(set0 + e)] == 1, "layer %d weight element not placed", l);
                }
            }
        }
    }
    for (size_t e = 0; e < elem.size(); ++e) CHECK(elem[e] != 0, "fragment element %zu is neither a weight nor a pad", e);
    std::vector<uint8_t> word((size_t)L.total_words, 0);
    for (int l = 0; l < L.n_layers; ++l) {
        const wn::Layer& y = L.l[l];
        CHECK(y.bias % 4 == 0, "bias alignment");
        for (int u = 0; u < 16 * y.nt; ++u) {
            const int64_t w = wn::bias_word(y, u);
            CHECK(w >= L.frag_words && w < L.w_words && word[(size_t)w] == 0, "layer %d bias %d", l, u);
            word[(size_t)w] = u < y.out ? 3 : 4;
        }
    }
    for (int64_t w = L.frag_words; w < L.w_words; ++w) CHECK(word[(size_t)w] != 0, "word %lld between the fragments and the status is unused", (long long)w);
    // ---- the act's LDS plan
    CHECK(L.tiles == 1 || L.tiles == 2 || L.tiles == 4, "tiles");
    CHECK(L.group == 16 * L.tiles && L.lds_bytes == 4 * L.lds_words && L.lds_bytes <= wn::kLdsMax, "LDS plan");
    CHECK(L.tiles == wn::kMaxTiles || wn::lds_words_at(L, 2 * L.tiles, nullptr) * 4 > wn::kLdsMax, "the plan takes the most tiles that fit");
    auto in_lds = [&](int64_t w) { return w >= 0 && w < L.lds_words; };
    auto region_of = [&](int64_t w) { return w >= L.region[1] ? 1 : 0; };
    for (int s = 0; s < L.n_layers; ++s) {
        CHECK(L.rs[s] % 4 == 0 && L.rs[s] >= wn::stage_cols(L, s), "stage %d row stride", s);
        for (int e = 0; e < L.group; ++e) {
            // the writes that define stage s (the staging: every column of the K-slices; layer s - 1: its tiles),
            // and layer s's 16-byte reads
            const int cols = s == 0 ? wn::stage_cols(L, 0) : 16 * L.l[s - 1].nt;
            CHECK(cols == wn::stage_cols(L, s), "stage %d: written and read columns differ", s);
            for (int k = 0; k < cols; ++k) {
                const int64_t w = wn::stage_word(L, s, e, k);
                CHECK(in_lds(w) && region_of(w) == (s & 1), "stage %d env %d column %d outside its region", s, e, k);
            }
            for (int t = 0; t < L.l[s].kt; ++t)
                for (int g = 0; g < 4; ++g) {
                    const int64_t w = wn::stage_word(L, s, e, 32 * t + 8 * g);
                    CHECK(w % 4 == 0 && in_lds(w + 7) && region_of(w + 7) == (s & 1), "stage %d read", s);
                }
        }
        // rows do not overlap
        CHECK(wn::stage_word(L, s, 1, 0) - wn::stage_word(L, s, 0, 0) >= wn::stage_cols(L, s), "stage %d rows overlap", s);
    }
    CHECK(L.region[0] == 0 && L.region[1] % 4 == 0, "regions");
    CHECK(wn::act_grid(L, 1, 256) == 1 && wn::act_grid(L, (int64_t)L.group + 1, 256) == 2, "grid");
    CHECK(wn::act_grid(L, (int64_t)1 << 40, 256) <= 4 * 256, "grid bound");
    // ---- the learner's plan
    int32_t in[4], out[4];
    for (int l = 0; l < L.n_layers; ++l) {
        in[l] = L.l[l].in;
        out[l] = L.l[l].out;
    }
    const int batches[3] = {1, 65, 4096};
    for (int b : batches) {
        ll::Plan P;
        const char* m = ll::plan(L.n_layers, in, out, L.code_w, b, &P, wn::kMaxWidth);
        CHECK(!m, "the learner's plan refused batch %d: %s", b, m ? m : "");
        CHECK(P.pub.bytes > 0 && P.n_params >= weights / 2, "plan size");
    }
    printf("net %d", n.in);
    for (int i = 0; i < n.nh; ++i) printf("-%d", n.h[i]);
    printf("-%d: %d words, %d tiles, %d B of LDS\n", n.actions, L.total_words, L.tiles, L.lds_bytes);
}

int main() {
    const Net nets[] = {{294, 3, {256, 128, 64}, 5, DRL_QNET_INPUT_CODE}, {294, 1, {136, 0, 0}, 5, DRL_QNET_INPUT_OBS},
                        {6, 1, {8, 0, 0}, 1, DRL_QNET_INPUT_OBS},         {512, 3, {256, 256, 256}, 8, DRL_QNET_INPUT_OBS},
                        {150, 1, {256, 0, 0}, 5, DRL_QNET_INPUT_CODE}};
    for (const Net& n : nets) check_net(n);
    // the learner's plan: 256 at the wide limit, 264 refused there, 136 refused at the default limit
    {
        ll::Plan P;
        const int32_t in[2] = {294, 256}, out[2] = {256, 5};
        CHECK(!ll::plan(2, in, out, 0, 4096, &P, wn::kMaxWidth), "256 at the wide limit");
        CHECK(ll::plan(2, in, out, 0, 8, &P) != nullptr, "256 at the default limit must be refused");
        const int32_t in2[2] = {294, 264}, out2[2] = {264, 5};
        CHECK(ll::plan(2, in2, out2, 0, 8, &P, wn::kMaxWidth) != nullptr, "264 must be refused");
        const int32_t in3[2] = {294, 136}, out3[2] = {136, 5};
        CHECK(ll::plan(2, in3, out3, 0, 8, &P) != nullptr, "136 at the default limit must be refused");
        CHECK(!ll::plan(2, in3, out3, 0, 8, &P, wn::kMaxWidth), "136 at the wide limit");
    }
    // the description's limits
    {
        wn::Layout L;
        drl_widenet_desc d{294, 1, {264, 0, 0}, 5, DRL_QNET_INPUT_OBS};
        CHECK(wn::layout(&d, &L) != nullptr, "width 264");
        d.hidden[0] = 256;
        CHECK(!wn::layout(&d, &L), "width 256");
        CHECK(wn::layout(nullptr, &L) != nullptr, "NULL desc");
    }
    printf("OK\n");
    return 0;
}
