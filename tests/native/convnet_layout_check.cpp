// CPU check of the conv Q-network's packed image and LDS plan (dronerl_amd/csrc/convnet/
// dronerl_convnet_layout.h, the header the pack kernel and the host API share).  For every net of
// tests/test_convnet.py's table and for the corners of the limits:
//   * the element -> parameter map of every layer's fragments hits each weight exactly once, and every other
//     element (the K and N padding) maps to "zero";
//   * the folded flatten is a bijection onto torch's channel-major index co*H*W + oy*W + ox;
//   * the image's sections tile [0, packed_bytes) without overlap (packed_bytes = the largest offset + size);
//   * every LDS word the act kernel gathers or writes lies inside its region of the env block: gathers inside
//     the layer's haloed input map, outputs inside the next map's interior, the blocks inside the LDS size.
// Descriptions outside a limit must be refused with a message that names the field.  Stand-alone host code
// (no HIP), built and run by tests/test_convnet_layout.py under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../dronerl_amd/csrc/convnet/dronerl_convnet_layout.h"

using drl::cv::Layer;
using drl::cv::Layout;

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

static int check(const char* name, const drl_convnet_desc& d) {
    Layout L;
    int bad = 0;
    const char* msg = drl::cv::layout(&d, &L);
    if (msg) {
        printf("%s: refused: %s\n", name, msg);
        return 1;
    }
    // map sides (floor division) and GEMM sizes
    int side = d.window, cin = 6;
    for (int i = 0; i < d.n_conv; ++i) {
        const Layer& y = L.l[i];
        EXPECT(y.conv && y.in_side == side && y.cin == cin && y.pad_side == side + 2 * y.p);
        EXPECT(y.out_side == (side + 2 * y.p - y.k) / y.s + 1 && y.out_side >= 1);
        EXPECT(y.K == y.k * y.k * cin && y.N == y.cout);
        side = y.out_side;
        cin = y.cout;
    }
    EXPECT(L.flat == side * side * cin);
    EXPECT(L.n_layers == d.n_conv + d.n_dense + 1 && L.l[L.n_layers - 1].N == d.n_actions);
    // the element -> parameter map
    for (int l = 0; l < L.n_layers; ++l) {
        const Layer& y = L.l[l];
        EXPECT(y.kt * 32 >= y.K && (y.kt - 1) * 32 < y.K && y.nt * 16 >= y.N && (y.nt - 1) * 16 < y.N);
        std::vector<int> hits((size_t)y.K * y.N, 0);
        const int64_t n = (int64_t)y.nt * y.kt * 512;
        int64_t pads = 0;
        for (int64_t e = 0; e < n; ++e) {
            int kk, nn;
            drl::cv::frag_elem(y, e, &kk, &nn);
            EXPECT(kk >= 0 && kk < 32 * y.kt && nn >= 0 && nn < 16 * y.nt);
            const int64_t idx = drl::cv::weight_index(L, l, kk, nn);
            if (kk >= y.K || nn >= y.N) {
                EXPECT(idx == -1);  // padding: the pack kernel writes zero
                ++pads;
                continue;
            }
            EXPECT(idx >= 0 && idx < (int64_t)y.K * y.N);
            if (idx >= 0 && idx < (int64_t)y.K * y.N) hits[(size_t)idx]++;
            if (y.conv) {  // the gather table reads the input the weight multiplies
                const int tap = kk / y.cin, ci = kk % y.cin, ky = tap / y.k, kx = tap % y.k;
                EXPECT(idx == (((int64_t)nn * y.cin + ci) * y.k + ky) * y.k + kx);
                EXPECT(drl::cv::tap_value(y, kk) == (ky * y.pad_side + kx) * y.cin + ci);
            } else if (l > L.n_conv) {
                EXPECT(idx == (int64_t)nn * y.K + kk);
            }
        }
        for (int v : hits) EXPECT(v == 1);
        EXPECT(pads == n - (int64_t)y.K * y.N);
        for (int kk = y.K; kk < 32 * y.kt; ++kk) EXPECT(drl::cv::tap_value(y, kk) == 0);
    }
    {  // the folded flatten: kernel order pos * cout + co -> torch's co * H * W + pos, a bijection
        const Layer& c = L.l[L.n_conv - 1];
        const int hw = c.out_side * c.out_side;
        std::vector<int> seen((size_t)L.flat, 0);
        for (int pos = 0; pos < hw; ++pos)
            for (int co = 0; co < c.cout; ++co) {
                const int t = drl::cv::flat_torch_index(L, pos * c.cout + co);
                EXPECT(t == co * hw + pos);
                if (t >= 0 && t < L.flat) seen[(size_t)t]++;
            }
        for (int v : seen) EXPECT(v == 1);
    }
    {  // the image's sections tile it
        std::vector<std::pair<int64_t, int64_t>> sec;
        for (int l = 0; l < L.n_layers; ++l) {
            const Layer& y = L.l[l];
            const int64_t setw = (int64_t)y.nt * y.kt * 256;
            sec.push_back({(int64_t)y.frag_hi * 4, setw});
            sec.push_back({(int64_t)y.frag_lo * 4, setw});
            sec.push_back({y.bias, y.nt * 16});
            if (y.conv) {
                sec.push_back({y.tap, y.kt * 32});
                sec.push_back({y.pin, y.mtiles * 16});
                sec.push_back({y.pout, y.mtiles * 16});
            }
        }
        sec.push_back({L.st_obs, (d.window * d.window * 3 + 3) / 4 * 4});
        sec.push_back({L.st_code, (d.window * d.window + 3) / 4 * 4});
        EXPECT(L.status == L.w_words && L.status % 4 == 0);
        sec.push_back({L.status, 4});
        std::sort(sec.begin(), sec.end());
        int64_t pos = 0;
        for (auto& s : sec) {
            EXPECT(s.first == pos && s.first % 4 == 0);
            pos = s.first + s.second;
        }
        EXPECT(pos == L.total_words);  // packed_bytes = the largest offset + size
    }
    {  // the LDS plan
        EXPECT(L.group >= 1 && L.group <= 16 && L.lds_bytes <= 160 * 1024 && L.env_words % 32 == 4);
        const int64_t wl = L.w_lds ? (int64_t)(L.w_words + 3) / 4 * 16 : 0;
        EXPECT(L.lds_bytes == wl + (int64_t)L.group * L.env_words * 4);
        std::vector<int> owner((size_t)L.env_words, -1);  // region of every word of an env's block
        for (int l = 0; l < L.n_layers; ++l) {
            const Layer& y = L.l[l];
            const int size = y.conv ? y.pad_side * y.pad_side * y.cin : y.kt * 32;
            EXPECT(y.in_reg >= 0 && y.in_reg + size <= L.env_words);
            if (!y.conv) EXPECT(y.in_reg % 4 == 0);
            for (int w = y.in_reg; w < y.in_reg + size && w < L.env_words; ++w) {
                EXPECT(owner[(size_t)w] == -1);
                owner[(size_t)w] = l;
            }
        }
        EXPECT(L.q_reg % 4 == 0 && L.q_reg + 8 <= L.env_words);
        for (int w = L.q_reg; w < L.q_reg + 8 && w < L.env_words; ++w) {
            EXPECT(owner[(size_t)w] == -1);
            owner[(size_t)w] = 100;
        }
        for (int l = 0; l < L.n_layers; ++l) {
            const Layer& y = L.l[l];
            if (!y.conv) {
                for (int u = 0; u < y.N; ++u) {
                    const int w = y.out_reg + u;
                    EXPECT(w >= 0 && w < L.env_words && owner[(size_t)w] == (l + 1 < L.n_layers ? l + 1 : 100));
                }
                continue;
            }
            // the position tables: item / mtiles as a multiply; every gather of every row of every M-tile (the
            // rows past the map included) stays inside this layer's map
            const int size = y.pad_side * y.pad_side * y.cin, hw = y.out_side * y.out_side;
            EXPECT(y.mtiles == (hw + 15) / 16);
            for (uint32_t item = 0; item < 16u * (uint32_t)y.mtiles; ++item)
                EXPECT((y.mtiles > 1 ? (uint32_t)(((uint64_t)item * (uint32_t)y.mt_magic) >> 32) : item) ==
                       item / (uint32_t)y.mtiles);
            for (int m = 0; m < 16 * y.mtiles; ++m) {
                const int oy = m / y.out_side, ox = m % y.out_side, base = drl::cv::pin_value(y, m);
                EXPECT(base == (m < hw ? (oy * y.s * y.pad_side + ox * y.s) * y.cin : 0));
                EXPECT(drl::cv::pout_value(y, m) == (m < hw ? (oy * y.out_row + ox) * y.cout : -1));
                for (int kk = 0; kk < 32 * y.kt; ++kk) {
                    const int w = base + drl::cv::tap_value(y, kk);
                    EXPECT(w >= 0 && w < size);
                }
            }
            // every output lands in the next layer's input: a conv map's interior, or the flatten
            const Layer& nx = L.l[l + 1];
            std::vector<int> wrote((size_t)L.env_words, 0);
            for (int oy = 0; oy < y.out_side; ++oy)
                for (int ox = 0; ox < y.out_side; ++ox)
                    for (int co = 0; co < y.cout; ++co) {
                        const int w = y.out_reg + drl::cv::pout_value(y, oy * y.out_side + ox) + co;
                        EXPECT(w >= 0 && w < L.env_words && owner[(size_t)w] == l + 1);
                        if (w >= 0 && w < L.env_words) wrote[(size_t)w]++;
                        if (nx.conv)
                            EXPECT(w == nx.in_reg + (((oy + nx.p) * nx.pad_side) + ox + nx.p) * nx.cin + co);
                        else
                            EXPECT(w == nx.in_reg + (oy * y.out_side + ox) * y.cout + co);
                    }
            for (int v : wrote) EXPECT(v <= 1);
        }
        // the staged window: layer 0's interior
        const Layer& y0 = L.l[0];
        const int org = y0.in_reg + (y0.p * y0.pad_side + y0.p) * 6, W = d.window;
        for (int i = 0; i < W * W * 6; ++i) {  // obs: float i of the row = channel i % 6 of cell i / 6
            const int w = org + drl::cv::st_obs_value(y0, W, i / 2) + (i & 1);
            EXPECT(w == y0.in_reg + (((i / 6) / W + y0.p) * y0.pad_side + (i / 6) % W + y0.p) * 6 + i % 6);
            EXPECT(w >= 0 && w < L.env_words && owner[(size_t)w] == 0);
        }
        std::vector<int> src_seen(4 * 24, 0);
        const int cpg = (W * W + 3) / 4, cpg8 = (cpg + 7) / 8 * 8;
        for (int cl = 0; cl < W * W; ++cl) {  // code: cell cl's u16 and its six words
            const int sd = drl::cv::st_code_value(y0, W, cl), src = sd & 0xffff, w = org + (sd >> 16);
            EXPECT(src == (cl / cpg) * cpg8 + cl % cpg && src < 4 * cpg8 && src_seen[(size_t)src]++ == 0);
            EXPECT(w == y0.in_reg + ((cl / W + y0.p) * y0.pad_side + cl % W + y0.p) * 6);
            EXPECT(w >= 0 && w + 5 < L.env_words && owner[(size_t)w] == 0 && owner[(size_t)w + 5] == 0);
        }
        for (uint32_t n = 0; n < 16u * (uint32_t)(W * W * 3); ++n) {
            EXPECT((uint32_t)(((uint64_t)n * (uint32_t)L.npair_magic) >> 32) == n / (uint32_t)(W * W * 3));
            if (n < 16u * (uint32_t)(W * W))
                EXPECT((uint32_t)(((uint64_t)n * (uint32_t)L.cells_magic) >> 32) == n / (uint32_t)(W * W));
        }
    }
    printf("%s: flat %d, image %d B, LDS %d B (%d envs%s): %d bad\n", name, L.flat, L.total_words * 4, L.lds_bytes,
           L.group, L.w_lds ? ", image staged" : "", bad);
    return bad;
}

static int refused(const char* field, const drl_convnet_desc& d) {
    Layout L;
    const char* msg = drl::cv::layout(&d, &L);
    if (!msg || !strstr(msg, field)) {
        printf("limit %s: %s\n", field, msg ? msg : "accepted");
        return 1;
    }
    return 0;
}

int main() {
    int total = 0;
    // tests/test_convnet.py's nets
    total += check("a", make(7, {{4, 3, 1, 1}}, {8}));
    total += check("b", make(7, {{8, 3, 1, 1}}, {}));
    total += check("c", make(9, {{8, 3, 1, 0}, {12, 3, 2, 1}}, {16, 8}));
    total += check("d", make(5, {{5, 5, 1, 2}}, {128}));
    total += check("e", make(3, {{32, 1, 1, 0}}, {8}));
    total += check("f", make(7, {{6, 2, 3, 0}}, {}));
    // the corners of the limits
    total += check("min", make(3, {{1, 1, 1, 0}}, {}, 1));
    total += check("k5s3p4", make(9, {{32, 5, 3, 4}, {32, 5, 1, 4}, {32, 5, 2, 0}}, {128, 128}, 8));
    total += check("wide", make(9, {{32, 1, 1, 4}}, {128}, 8));
    total += check("grow", make(9, {{8, 1, 1, 4}, {8, 1, 1, 2}}, {8}));        // maps that grow: 9 -> 17 -> 21
    total += check("one", make(3, {{7, 3, 1, 0}}, {8}));                       // a 1x1 map
    total += check("code9", make(9, {{8, 4, 2, 1}}, {24}, 5, DRL_QNET_INPUT_CODE));
    total += check("three", make(9, {{3, 2, 1, 0}, {17, 3, 1, 1}, {9, 4, 2, 2}}, {40}));
    // outside a limit: refused, the message names the field
    total += refused("window", make(4, {{4, 3, 1, 1}}, {8}));
    total += refused("window", make(11, {{4, 3, 1, 1}}, {8}));
    total += refused("window", make(1, {{4, 1, 1, 0}}, {8}));
    total += refused("n_conv", make(7, {}, {8}));
    total += refused("n_conv", make(7, {{4, 3, 1, 1}, {4, 3, 1, 1}, {4, 3, 1, 1}, {4, 3, 1, 1}}, {8}));
    total += refused("out_channels", make(7, {{0, 3, 1, 1}}, {8}));
    total += refused("out_channels", make(7, {{33, 3, 1, 1}}, {8}));
    total += refused("kernel_size", make(7, {{4, 0, 1, 1}}, {8}));
    total += refused("kernel_size", make(7, {{4, 6, 1, 1}}, {8}));
    total += refused("stride", make(7, {{4, 3, 0, 1}}, {8}));
    total += refused("stride", make(7, {{4, 3, 4, 1}}, {8}));
    total += refused("padding", make(7, {{4, 3, 1, -1}}, {8}));
    total += refused("padding", make(7, {{4, 3, 1, 5}}, {8}));
    total += refused("map side", make(3, {{4, 5, 1, 0}}, {8}));
    total += refused("n_dense", make(7, {{4, 3, 1, 1}}, {8, 8, 8}));
    total += refused("dense widths", make(7, {{4, 3, 1, 1}}, {12}));
    total += refused("dense widths", make(7, {{4, 3, 1, 1}}, {136}));
    total += refused("n_actions", make(7, {{4, 3, 1, 1}}, {8}, 0));
    total += refused("n_actions", make(7, {{4, 3, 1, 1}}, {8}, 9));
    total += refused("input", make(7, {{4, 3, 1, 1}}, {8}, 5, 2));
    total += refused("input", make(3, {{4, 3, 1, 1}}, {8}, 5, DRL_QNET_INPUT_CODE));
    total += refused("LDS", make(9, {{32, 1, 1, 4}, {32, 1, 1, 4}, {32, 1, 1, 4}}, {8}));
    printf(total ? "FAIL\n" : "OK\n");
    return total ? 1 : 0;
}
