// dronerl_widenet_layout.h — wide dense Q-networks (include/dronerl.h drl_widenet_*): the description's
// validation, the packed image's layout and the act kernel's LDS plan and grid.  Plain C++ (no HIP): the host
// API, the kernels and tests/native/widenet_layout_check.cpp share it.  kMaxWidth is the one width limit.
//
// Every layer is a GEMM D[unit][env] = W[unit][k] * x[k][env] on v_mfma_f32_16x16x32_f16 with the weights as the
// A operand and a tile of 16 envs as B.  Fragment (n, t) of a layer (16-unit tile n, 32-wide K-slice t) is 64
// lanes x 8 fp16 elements: element j of lane (c = lane & 15, g = lane >> 4) is W[16 n + c][32 t + 8 g + j], zero
// where the unit or k is padding; the B operand's lane (c, g) holds env c's inputs 32 t + 8 g + j, and the
// accumulator's register i of lane (c, g) is unit 16 n + 4 g + i of env c.  A layer has a hi set (fp16(w)) and
// a lo set (fp16((w - hi) * 2^11)) of nt * kt fragments each; one 16-byte load per lane reads a fragment.
//
// The image (32-bit words): every layer's hi set, then its lo set; every layer's f32 biases (16 nt floats, zero
// pads); a 16-byte status vector (word 0: DRL_ERR_QNET_RANGE when a packed weight is outside fp16's range).
//
// The act's LDS: a workgroup takes `group` = 16 * tiles envs per pass.  Activation stage s (0: the input, s: layer
// s - 1's outputs) is one 32-bit word per value, already split (fp16 hi in the low half, lo in the high one), in
// rows of rs[s] = 32 kt[s] + 4 words (= 4 mod 32: the lanes' 16-byte row reads and writes spread over the banks).
// Even stages live in region 0, odd ones in region 1 (a layer reads one region and writes the other); region r
// holds `group` rows of its widest stage.  The Q head's values go from registers to the epilogue.
#ifndef DRONERL_WIDENET_LAYOUT_H
#define DRONERL_WIDENET_LAYOUT_H

#include <stdint.h>

#include "../../../include/dronerl.h"

#if defined(__HIPCC__)
#define DRL_WN_HD __host__ __device__ inline
#else
#define DRL_WN_HD inline
#endif

namespace drl {
namespace wn {

constexpr int kMaxWidth = DRL_WIDENET_MAX_WIDTH;  // the width limit (hidden widths; the learner's plan takes it too)
constexpr int kMaxIn = 512, kMaxActions = 8;
constexpr int kMaxLayers = 4;                     // up to 3 hidden layers and the Q head
constexpr int kLdsMax = 160 * 1024;
constexpr int kWaves = 8, kThreads = 64 * kWaves;  // the act's workgroup
constexpr int kMaxTiles = 4;                       // 16-env tiles per workgroup pass: 4, 2 or 1 by the LDS plan

struct Layer {
    int32_t in, out;           // the logical sizes
    int32_t kt, nt;            // 32-wide K-slices; 16-unit tiles (a hidden layer: an even count, so its outputs fill
                               // the next layer's K-slices and the pad units' zeros are its K padding)
    int32_t frag_hi, frag_lo;  // 16-B vectors from the image's start: fragment (n, t) at + (n * kt + t) * 64 + lane
    int32_t bias;              // words from the image's start: 16 nt floats
};

struct Layout {
    int32_t n_layers, n_actions, input, code_w;  // code_w > 0: a policy-code net of a code_w x code_w window
    int32_t frag_words;   // words of all fragments (the biases follow)
    int32_t w_words;      // words before the status vector (what the pack kernel writes)
    int32_t status;       // words from the image's start: the 16-B pack status
    int32_t total_words;
    // the act's plan
    int32_t tiles, group;          // 16-env tiles and envs per workgroup pass
    int32_t rs[kMaxLayers];        // stage s's row stride in words (stage s is layer s's input)
    int32_t region[2];             // words from the LDS start of the even / odd stages' region
    int32_t lds_words, lds_bytes;
    int32_t cells_magic;           // code input: index / (code_w * code_w) as a multiply
    int32_t pairs_magic;           // obs input: index / (16 kt[0]) as a multiply (a row's float pairs, pads included)
    Layer l[kMaxLayers];
};

// n / d == umulhi(n, magic(d)) exactly for n * d < 2^32 and d > 1
inline int32_t fastdiv_magic(int d) { return d > 1 ? (int32_t)(uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0; }

// LDS words of the plan at `tiles` tiles per pass
inline int64_t lds_words_at(const Layout& L, int tiles, int32_t* region) {
    int64_t w[2] = {0, 0};
    for (int s = 0; s < L.n_layers; ++s) w[s & 1] = L.rs[s] > w[s & 1] ? L.rs[s] : w[s & 1];
    const int64_t g = 16 * tiles;
    if (region) {
        region[0] = 0;
        region[1] = (int32_t)(g * w[0]);
    }
    return g * (w[0] + w[1]);
}

// Validate a description and lay the net out.  Returns nullptr, or the message for drl_last_error.
inline const char* layout(const drl_widenet_desc* d, Layout* L) {
    if (!d) return "widenet desc is NULL";
    if (!L) return "internal: the widenet layout's output is NULL";
    if (d->in_features < 2 || d->in_features > kMaxIn || (d->in_features & 1))
        return "in_features must be even and in [2, 512]";
    if (d->n_hidden < 1 || d->n_hidden > 3) return "n_hidden must be 1, 2 or 3";
    for (int i = 0; i < d->n_hidden; ++i)
        if (d->hidden[i] < 8 || d->hidden[i] > kMaxWidth || d->hidden[i] % 8)
            return "hidden widths must be multiples of 8 in [8, 256] (DRL_WIDENET_MAX_WIDTH)";
    if (d->n_actions < 1 || d->n_actions > kMaxActions) return "n_actions must be in [1, 8]";
    int code_w = 0;
    if (d->input == DRL_QNET_INPUT_CODE) {
        for (int w = 5; w <= 9; w += 2)
            if (d->in_features == w * w * 6) code_w = w;
        if (!code_w) return "input: a policy-code net takes a 5x5, 7x7 or 9x9 window (in_features W*W*6)";
    } else if (d->input != DRL_QNET_INPUT_OBS) {
        return "input must be DRL_QNET_INPUT_OBS or DRL_QNET_INPUT_CODE";
    }
    *L = Layout{};
    L->n_layers = d->n_hidden + 1;
    L->n_actions = d->n_actions;
    L->input = d->input;
    L->code_w = code_w;
    int vec = 0;
    for (int l = 0; l < L->n_layers; ++l) {
        Layer& y = L->l[l];
        y.in = l == 0 ? d->in_features : d->hidden[l - 1];
        y.out = l < d->n_hidden ? d->hidden[l] : d->n_actions;
        y.kt = (y.in + 31) / 32;
        y.nt = l < d->n_hidden ? 2 * ((y.out + 31) / 32) : 1;
        y.frag_hi = vec;
        y.frag_lo = vec + y.nt * y.kt * 64;
        vec += 2 * y.nt * y.kt * 64;
        L->rs[l] = 32 * y.kt + 4;
    }
    L->frag_words = vec * 4;
    int w = L->frag_words;
    for (int l = 0; l < L->n_layers; ++l) {
        L->l[l].bias = w;
        w += 16 * L->l[l].nt;
    }
    L->w_words = w;
    L->status = w;  // (a multiple of 4 words: 16-byte aligned)
    L->total_words = w + 4;
    // the most tiles per pass whose two regions fit the LDS: each weight fragment read serves all of them
    int tiles = kMaxTiles;
    while (tiles > 1 && lds_words_at(*L, tiles, nullptr) * 4 > kLdsMax) tiles /= 2;
    L->tiles = tiles;
    L->group = 16 * tiles;
    L->lds_words = (int32_t)lds_words_at(*L, tiles, L->region);
    L->lds_bytes = L->lds_words * 4;
    if (L->lds_bytes > kLdsMax) return "internal: the wide act's activations do not fit the LDS of a CU";
    L->cells_magic = code_w ? fastdiv_magic(code_w * code_w) : 0;
    L->pairs_magic = fastdiv_magic(16 * L->l[0].kt);
    return nullptr;
}

// ---- the image ------------------------------------------------------------------------------------------------
// fp16 element e (from the start of layer y's hi or lo set: fragment, lane, j) -> the weight W[unit][k] it
// holds; a unit >= out or a k >= in is a zero pad
DRL_WN_HD void frag_elem(const Layer& y, int64_t e, int* unit, int* k) {
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
    const int64_t frag = e >> 9;
    const int n = (int)(frag / y.kt), t = (int)(frag - (int64_t)n * y.kt);
    *unit = 16 * n + (lane & 15);
    *k = 32 * t + 8 * (lane >> 4) + j;
}
// The inverse: W[unit][k]'s fp16 element in the whole image (piece 0: hi, 1: lo), 2 per word
DRL_WN_HD int64_t weight_elem(const Layer& y, int unit, int k, int piece) {
    const int n = unit >> 4, c = unit & 15, t = k >> 5, g = (k >> 3) & 3, j = k & 7;
    const int64_t e = ((((int64_t)n * y.kt + t) * 64) + (g * 16 + c)) * 8 + j;
    return (int64_t)(piece ? y.frag_lo : y.frag_hi) * 8 + e;
}
DRL_WN_HD int64_t bias_word(const Layer& y, int unit) { return (int64_t)y.bias + unit; }

// ---- the act's LDS --------------------------------------------------------------------------------------------
// word of value k of stage s of the pass's env e
DRL_WN_HD int stage_word(const Layout& L, int s, int e, int k) { return L.region[s & 1] + e * L.rs[s] + k; }
// the columns of stage s a pass defines (written before layer s reads them): all of its K-slices
DRL_WN_HD int stage_cols(const Layout& L, int s) { return 32 * L.l[s].kt; }

// workgroups of the act: one pass per group of envs, at most per_cu resident workgroups per CU
inline int64_t act_grid(const Layout& L, int64_t E, int num_cus) {
    const int64_t ngroups = (E + L.group - 1) / L.group;
    int per_cu = kLdsMax / L.lds_bytes;
    per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
    const int64_t nb = (int64_t)num_cus * per_cu;
    return nb < ngroups ? nb : ngroups;
}

// ---- kernel arguments (dronerl_widenet.hip; launched by dronerl_widenet_api.cpp) --------------------------------
struct PackArgs {
    Layout L;
    const float* w[kMaxLayers];
    const float* b[kMaxLayers];
    uint32_t* packed;
};

// (the field names dronerl_act_common.h's functions read are the other acts')
struct ActArgs {
    Layout L;
    const uint32_t* packed;
    const void* input;
    int64_t obs_stride, E;
    float epsilon;
    const float* eps_ptr;
    uint64_t seed, step;
    int64_t env_offset;
    int32_t* actions;
    int64_t action_stride;
    float* q;
    int32_t* err;
    int32_t n_actions;
};

// (hipError_t values)
int launch_widenet_pack(const PackArgs& a, hipStream_t s);
int launch_widenet_act(const ActArgs& a, int num_cus, hipStream_t s);

}  // namespace wn
}  // namespace drl
#endif
