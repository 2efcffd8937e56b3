// dronerl_convnet_layout.h — shape arithmetic of the conv Q-network (include/dronerl.h drl_convnet_*): map
// sides, the K and N padding of every layer's GEMM, the offsets inside the packed image, the element ->
// parameter map of the pack kernel and the folded flatten permutation.  Plain C++ (no HIP): the host API, the
// pack kernel and tests/native/convnet_layout_check.cpp share it.
//
// Every layer is a GEMM D[M][N] = A[M][K] * B[K][N] on v_mfma_f32_16x16x32_f16: A the activations (conv: M =
// output positions of one env, K = (tap, in channel); dense: M = envs, K = the previous layer's outputs), B the
// weights, packed here as lane fragments.  Fragment (n, t) of a layer (N-tile n, K-slice t) is 64 lanes x 8 fp16
// elements; element j of lane (c = lane & 15, g = lane >> 4) is B[32 t + 8 g + j][16 n + c] (the A operand's lane
// (c, g) holds A[row c][32 t + 8 g + j]: both index K by (g, j), so this K order is ours to choose).
#ifndef DRONERL_CONVNET_LAYOUT_H
#define DRONERL_CONVNET_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"

#if defined(__HIPCC__)
#define DRL_CV_HD __host__ __device__ inline
#else
#define DRL_CV_HD inline
#endif

namespace drl {
namespace cv {

constexpr int kMaxConv = DRL_CONVNET_MAX_CONV;       // 3
constexpr int kMaxDense = DRL_CONVNET_MAX_DENSE + 1;  // hidden dense layers + the Q head
constexpr int kMaxLayers = kMaxConv + kMaxDense;
constexpr int kGroupMax = 16;                         // envs per workgroup pass (one MFMA M-tile of the dense tail)
constexpr int kLdsMax = 160 * 1024;
constexpr int kWeightLdsMax = 40 * 1024;              // the fragments are staged in LDS up to this size

struct Layer {
    int32_t conv;            // 1: a conv layer; 0: dense
    int32_t K, N;            // the GEMM's reduce and output sizes (conv: k*k*cin, cout)
    int32_t kt, nt;          // 32-wide K-slices, 16-wide N-tiles
    int32_t frag_hi, frag_lo;  // 16-B vectors from the image's start: fragment (n, t) at + (n * kt + t) * 64 + lane
    int32_t bias;            // 32-bit words from the image's start: nt * 16 floats
    int32_t tap;             // conv: words from the image's start of the K-slot -> LDS offset table (kt * 32 ints)
    // conv: the items' M-tiles (16 output positions each), item / mtiles as a multiply (fastdiv_magic), and two
    // tables of mtiles * 16 ints (words from the image's start): an output position's top-left input word in the
    // staged map (pin_value) and its output's word before the channel (pout_value; -1 past the map)
    int32_t mtiles, mt_magic, pin, pout;
    int32_t cin, cout, k, s, p;
    int32_t in_side, out_side, pad_side;  // pad_side = in_side + 2 p: the staged map with its zero halo
    int32_t in_reg;          // words from an env's LDS block: this layer's input
    // where the outputs go (words from the env's block): conv: out_reg + ((oy * out_row) + ox) * cout + co, which
    // lands inside the next conv layer's halo (out_reg includes its padding offset) or is the position-major
    // flatten; dense: out_reg + unit
    int32_t out_reg, out_row;
};

struct Layout {
    int32_t n_conv, n_layers, window, input, n_actions;
    int32_t flat;        // the flatten's size: out_side^2 * cout of the last conv layer
    int32_t env_words;   // LDS words per env (= 4 mod 32: the dense tail's 16-B row reads spread over the banks)
    int32_t q_reg;       // words from an env's block: the Q head's f32 outputs (8)
    int32_t group;       // envs per workgroup pass
    int32_t w_lds;       // 1: the fragments, biases and tap tables are staged in LDS (w_words words, at 0)
    int32_t w_words;     // words of the image before the status vector
    int32_t status;      // words from the image's start: the 16-B pack status
    int32_t total_words;
    int32_t lds_bytes;
    // the staging tables (words from the image's start): float pair -> word of layer 0's map (st_obs_value, W*W*3
    // entries), window cell -> its u16 in the policy code row | its first word of the map << 16 (st_code_value,
    // W*W entries); and index / entries as multiplies
    int32_t st_obs, st_code, npair_magic, cells_magic;
    Layer l[kMaxLayers];
};

inline int conv_out_side(int side, int k, int s, int p) { return (side + 2 * p - k) / s + 1; }
// n / d == umulhi(n, fastdiv_magic(d)) exactly for n * d < 2^32 and d > 1 (d == 1: 0, the caller takes n)
inline int32_t fastdiv_magic(int d) { return d > 1 ? (int32_t)(uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0; }

// Validate a description and lay the net out.  Returns nullptr, or the message for drl_last_error.
inline const char* layout(const drl_convnet_desc* d, Layout* L) {
    if (!d) return "convnet desc is NULL";
    if (d->window < 3 || d->window > 9 || !(d->window & 1)) return "window must be odd and in [3, 9]";
    if (d->n_conv < 1 || d->n_conv > kMaxConv) return "n_conv must be 1, 2 or 3";
    if (d->n_dense < 0 || d->n_dense > DRL_CONVNET_MAX_DENSE) return "n_dense must be 0, 1 or 2";
    for (int i = 0; i < d->n_dense; ++i)
        if (d->dense[i] < 8 || d->dense[i] > 128 || d->dense[i] % 8)
            return "dense widths must be multiples of 8 in [8, 128]";
    if (d->n_actions < 1 || d->n_actions > 8) return "n_actions must be in [1, 8]";
    if (d->input == DRL_QNET_INPUT_CODE) {
        if (d->window < 5) return "input: a policy-code net takes a 5x5, 7x7 or 9x9 window";
    } else if (d->input != DRL_QNET_INPUT_OBS) {
        return "input must be DRL_QNET_INPUT_OBS or DRL_QNET_INPUT_CODE";
    }
    *L = Layout{};
    L->n_conv = d->n_conv;
    L->n_layers = d->n_conv + d->n_dense + 1;
    L->window = d->window;
    L->input = d->input;
    L->n_actions = d->n_actions;
    int side = d->window, cin = 6;
    for (int i = 0; i < d->n_conv; ++i) {
        const drl_convnet_conv& c = d->conv[i];
        if (c.out_channels < 1 || c.out_channels > 32) return "out_channels must be in [1, 32]";
        if (c.kernel_size < 1 || c.kernel_size > 5) return "kernel_size must be in [1, 5]";
        if (c.stride < 1 || c.stride > 3) return "stride must be in [1, 3]";
        if (c.padding < 0 || c.padding > 4) return "padding must be in [0, 4]";
        if (side + 2 * c.padding < c.kernel_size) return "kernel_size is larger than the padded map (every map side must be >= 1)";
        Layer& y = L->l[i];
        y.conv = 1;
        y.cin = cin;
        y.cout = c.out_channels;
        y.k = c.kernel_size;
        y.s = c.stride;
        y.p = c.padding;
        y.in_side = side;
        y.pad_side = side + 2 * c.padding;
        y.out_side = conv_out_side(side, c.kernel_size, c.stride, c.padding);
        y.K = y.k * y.k * cin;
        y.N = y.cout;
        side = y.out_side;
        cin = y.cout;
    }
    L->flat = side * side * cin;
    for (int i = d->n_conv; i < L->n_layers; ++i) {
        Layer& y = L->l[i];
        y.K = i == d->n_conv ? L->flat : L->l[i - 1].N;
        y.N = i + 1 < L->n_layers ? d->dense[i - d->n_conv] : d->n_actions;
    }
    // the image: hi and lo fragments of every layer, the biases, the tap tables, the position and staging
    // tables, the status vector
    int64_t vec = 0;
    for (int i = 0; i < L->n_layers; ++i) {
        Layer& y = L->l[i];
        y.kt = (y.K + 31) / 32;
        y.nt = (y.N + 15) / 16;
        y.frag_hi = (int32_t)vec;
        vec += (int64_t)y.nt * y.kt * 64;
        y.frag_lo = (int32_t)vec;
        vec += (int64_t)y.nt * y.kt * 64;
    }
    int64_t word = vec * 4;
    for (int i = 0; i < L->n_layers; ++i) {
        L->l[i].bias = (int32_t)word;
        word += L->l[i].nt * 16;
    }
    for (int i = 0; i < L->n_conv; ++i) {
        L->l[i].tap = (int32_t)word;
        word += L->l[i].kt * 32;
    }
    for (int i = 0; i < L->n_conv; ++i) {
        Layer& y = L->l[i];
        y.mtiles = (y.out_side * y.out_side + 15) / 16;
        y.mt_magic = fastdiv_magic(y.mtiles);
        y.pin = (int32_t)word;
        word += y.mtiles * 16;
        y.pout = (int32_t)word;
        word += y.mtiles * 16;
    }
    L->st_obs = (int32_t)word;
    word += (d->window * d->window * 3 + 3) / 4 * 4;
    L->st_code = (int32_t)word;
    word += (d->window * d->window + 3) / 4 * 4;
    L->npair_magic = fastdiv_magic(d->window * d->window * 3);
    L->cells_magic = fastdiv_magic(d->window * d->window);
    L->w_words = (int32_t)word;
    L->status = (int32_t)word;
    L->total_words = (int32_t)word + 4;
    // an env's LDS block: each conv layer's input map with its halo, the flatten, each hidden dense layer's
    // outputs (every dense input padded with zero words to whole K-slices), the Q values
    int64_t reg = 0;
    for (int i = 0; i < L->n_layers; ++i) {
        Layer& y = L->l[i];
        if (!y.conv) reg = (reg + 3) / 4 * 4;  // (a dense layer reads its rows as 16-B vectors)
        y.in_reg = (int32_t)reg;
        reg += y.conv ? (int64_t)y.pad_side * y.pad_side * y.cin : (int64_t)y.kt * 32;
    }
    L->q_reg = (int32_t)reg;
    reg += 8;
    for (int i = 0; i < L->n_layers; ++i) {
        Layer& y = L->l[i];
        if (!y.conv) {
            y.out_reg = i + 1 < L->n_layers ? L->l[i + 1].in_reg : L->q_reg;
        } else if (L->l[i + 1].conv) {
            const Layer& nx = L->l[i + 1];
            y.out_row = nx.pad_side;
            y.out_reg = nx.in_reg + (nx.p * nx.pad_side + nx.p) * y.cout;
        } else {
            y.out_row = y.out_side;
            y.out_reg = L->l[i + 1].in_reg;
        }
    }
    reg += ((4 - reg) % 32 + 32) % 32;
    L->env_words = (int32_t)reg;
    if (reg * 4 > kLdsMax) return "the network's maps do not fit the 160 KB LDS of a CU (window, padding and out_channels)";
    if (word >= ((int64_t)1 << 28)) return "the packed network is too large";
    L->w_lds = word * 4 <= kWeightLdsMax;
    const int64_t wl = L->w_lds ? (word + 3) / 4 * 16 : 0;
    L->group = kGroupMax;
    while (L->group > 1 && wl + (int64_t)L->group * reg * 4 > kLdsMax) L->group /= 2;
    if (wl + (int64_t)L->group * reg * 4 > kLdsMax) {
        L->w_lds = 0;
        L->lds_bytes = (int32_t)(L->group * reg * 4);
    } else {
        L->lds_bytes = (int32_t)(wl + (int64_t)L->group * reg * 4);
    }
    return nullptr;
}

// ---- the element -> parameter map -----------------------------------------------------------------------
// Index into the layer's weight tensor in torch layout (conv [out][in][kh][kw], dense [out][in]) of GEMM element
// B[kk][n], or -1 where the packed image holds a zero (the K and N padding).  The first dense layer's K runs over
// the conv activations as the act kernel leaves them, position-major (kk = pos * cout + co): its torch column
// is the channel-major flatten co * H * W + pos (flat_torch_index).
DRL_CV_HD int flat_torch_index(const Layout& L, int kk) {
    const Layer& c = L.l[L.n_conv - 1];
    const int hw = c.out_side * c.out_side;
    return (kk % c.cout) * hw + kk / c.cout;
}

DRL_CV_HD int64_t weight_index(const Layout& L, int layer, int kk, int n) {
    const Layer& y = L.l[layer];
    if (kk >= y.K || n >= y.N) return -1;
    if (y.conv) {
        const int tap = kk / y.cin, ci = kk % y.cin, ky = tap / y.k, kx = tap % y.k;
        return (((int64_t)n * y.cin + ci) * y.k + ky) * y.k + kx;
    }
    return (int64_t)n * y.K + (layer == L.n_conv ? flat_torch_index(L, kk) : kk);
}

// fp16 element e of a layer's hi (or lo) fragment set -> (kk, n)
DRL_CV_HD void frag_elem(const Layer& y, int64_t e, int* kk, int* n) {
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
    const int64_t f = e >> 9;
    const int t = (int)(f % y.kt), nn = (int)(f / y.kt);
    *kk = 32 * t + 8 * (lane >> 4) + j;
    *n = 16 * nn + (lane & 15);
}

// a conv layer's tap table: K slot kk -> words from the output position's top-left input word in the staged map
// (pad slots: 0, a valid word under a zero weight)
DRL_CV_HD int tap_value(const Layer& y, int kk) {
    if (kk >= y.K) return 0;
    const int tap = kk / y.cin, ci = kk % y.cin, ky = tap / y.k, kx = tap % y.k;
    return (ky * y.pad_side + kx) * y.cin + ci;
}

// a conv layer's position tables (entry m of mtiles * 16; the out_reg / out_row they use are laid out first)
DRL_CV_HD int pin_value(const Layer& y, int m) {
    const int mm = m < y.out_side * y.out_side ? m : 0;  // (a tile's rows past the map gather position 0's words)
    const int oy = mm / y.out_side, ox = mm % y.out_side;
    return (oy * y.s * y.pad_side + ox * y.s) * y.cin;
}
DRL_CV_HD int pout_value(const Layer& y, int m) {
    if (m >= y.out_side * y.out_side) return -1;
    return ((m / y.out_side) * y.out_row + m % y.out_side) * y.cout;
}
// the staging tables: words from the interior's first word of layer 0's map ([p][p][0])
DRL_CV_HD int st_obs_value(const Layer& y0, int window, int pr) {
    if (pr >= window * window * 3) return 0;
    const int i = 2 * pr, row = window * 6;  // (row is even: a pair stays in its row)
    return (i / row) * y0.pad_side * 6 + i % row;
}
// (the policy code's row: 4 groups of cpg = ceil(W*W / 4) cells, each padded to cpg8 u16 -- dronerl_internal.h
// lay::code_cpg / code_cpg8)
DRL_CV_HD int st_code_value(const Layer& y0, int window, int cl) {
    if (cl >= window * window) return 0;
    const int cpg = (window * window + 3) / 4, cpg8 = (cpg + 7) / 8 * 8;
    const int cg = cl / cpg, src = cg * cpg8 + (cl - cg * cpg);
    const int dst = ((cl / window) * y0.pad_side + cl % window) * 6;
    return src | (dst << 16);
}

// ---- kernel arguments (dronerl_convnet.hip; launched by dronerl_convnet_api.cpp) ---------------------------
struct PackArgs {
    Layout L;
    const float* w[kMaxLayers];  // conv layers, then dense layers (torch layouts)
    const float* b[kMaxLayers];
    uint32_t* packed;
};

struct ActArgs {
    Layout L;
    const uint32_t* packed;
    const void* input;     // f32 rows, or policy-code rows
    int64_t obs_stride;    // floats
    int64_t E;
    float epsilon;
    const float* eps_ptr;  // nullable
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;
    int64_t action_stride;
    float* q;              // nullable
    int32_t* err;          // nullable
};

// (hipError_t values)
int launch_convnet_pack(const PackArgs& a, hipStream_t s);
int launch_convnet_act(const ActArgs& a, int num_cus, hipStream_t s);

}  // namespace cv
}  // namespace drl
#endif
