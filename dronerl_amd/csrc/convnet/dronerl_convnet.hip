// dronerl_convnet.hip — convolutional Q-networks on the device, the inference half (include/dronerl.h
// drl_convnet_*): the pack kernel and the forward + epsilon-greedy act.
//
// Reference: torch_impl/agents/dqn.py:85-159 ConvQNetwork (Conv2d + ReLU per conv layer on [B][C][H][W],
// Flatten, Linear + ReLU per dense layer, Linear(n_actions)); jax_impl/agents/dqn.py:66-94 (the same net,
// channels last, transposed before the flatten); DQNAgent.act (jax dqn.py:132-146).
//
// Every layer is a GEMM on v_mfma_f32_16x16x32_f16 with DRL_QNET_F32's numerics (dronerl_qnet.hip split_f16:
// each operand v as fp16 hi = fp16(v) and lo = fp16((v - hi) * 2^11); acc += xhi * Whi, acl += xlo * Whi +
// xhi * Wlo; the layer's value is (acc + 2^-11 acl) + bias).  A workgroup stages a group of env windows in LDS
// with the first conv layer's zero halo, already split: one 32-bit word per value, hi in the low half and lo
// in the high one, so a value gathered k*k times is split once.  A conv layer is an implicit GEMM per env (M
// = output positions, N = out channels, K = (tap, in channel)): lane (c, g)'s A fragment of K-slice t is 8
// words gathered at [its position's top-left word] + tap[32 t + 8 g + j], the table the pack kernel wrote;
// the halo makes every gather in bounds without a branch.  Outputs go back to LDS, split, into the next conv
// layer's map (inside its halo) or position-major into the flatten, whose order the first dense layer's packed
// columns follow (no transpose).  The dense tail runs with M = the group's envs.  The layout arithmetic is
// dronerl_convnet_layout.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "dronerl_convnet_layout.h"

namespace drl {
namespace cv {

// (st_code_value restates the policy code's row geometry without HIP)
static_assert(lay::code_cpg(5) == 7 && lay::code_cpg8(5) == 8 && lay::code_cpg(7) == 13 && lay::code_cpg8(7) == 16 &&
              lay::code_cpg(9) == 21 && lay::code_cpg8(9) == 24, "policy code row geometry");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;

#define CV_MFMA __builtin_amdgcn_mfma_f32_16x16x32_f16

__device__ __forceinline__ uint32_t f16_bits(_Float16 h) {
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}

// v as one word: fp16 hi in bits 0-15, fp16 lo in bits 16-31 (split_f16's two pieces).  `bad`: |v| >= 65520
// rounds hi to inf, NaN stays NaN (DRL_ERR_QNET_RANGE).
__device__ __forceinline__ uint32_t split_word(float v, bool& bad) {
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)((v - (float)h) * 2048.0f);
    bad |= !(__builtin_fabsf(v) < 65520.0f);
    return f16_bits(h) | (f16_bits(l) << 16);
}

// 8 split words -> the hi and the lo MFMA operand
__device__ __forceinline__ void operands(const uint32_t (&d)[8], f16x8& hi, f16x8& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        h[p] = (d[2 * p] & 0xffffu) | (d[2 * p + 1] << 16);
        l[p] = (d[2 * p] >> 16) | (d[2 * p + 1] & 0xffff0000u);
    }
    __builtin_memcpy(&hi, h, 16);
    __builtin_memcpy(&lo, l, 16);
}

__device__ __forceinline__ f16x8 frag16(const uint32_t* w, int vec) {
    const uint4 v = reinterpret_cast<const uint4*>(w)[vec];
    f16x8 f;
    __builtin_memcpy(&f, &v, 16);
    return f;
}

// drl_obs's charge channel (dronerl_kernels.hip div100: c / 100 correctly rounded)
__device__ __forceinline__ float cv_div100(int c) {
    const float x = (float)c;
    const float r = 0.01f;
    const float q = x * r;
    const float e = __fmaf_rn(-q, 100.0f, x);
    return __fmaf_rn(e, r, q);
}

// ------------------------------------------------------------------ pack ---
// One thread per 32-bit word of the image: two fp16 fragment elements (hi or lo pieces of the weights
// weight_index names, zero in the K and N padding), a bias, or an entry of the tap, position or staging tables.
__global__ void __launch_bounds__(256) drl_convnet_pack_kernel(PackArgs a) {
    const Layout& L = a.L;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.w_words) return;
    if (i < L.l[0].bias) {
        int l = 0;
        while (l + 1 < L.n_layers && i >= (int64_t)L.l[l + 1].frag_hi * 4) ++l;
        const Layer& y = L.l[l];
        const int64_t setw = (int64_t)y.nt * y.kt * 256;  // words of one fragment set
        const int64_t r = i - (int64_t)y.frag_hi * 4;
        const bool lo = r >= setw;
        const int64_t e0 = (lo ? r - setw : r) * 2;
        uint32_t word = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int kk, n;
            frag_elem(y, e0 + h, &kk, &n);
            const int64_t idx = weight_index(L, l, kk, n);
            const float w = idx >= 0 ? a.w[l][idx] : 0.0f;
            if (!lo && !(__builtin_fabsf(w) < 65504.0f))
                atomicOr(reinterpret_cast<int32_t*>(a.packed + L.status), DRL_ERR_QNET_RANGE);
            const _Float16 hi = (_Float16)w;
            word |= f16_bits(lo ? (_Float16)((w - (float)hi) * 2048.0f) : hi) << (16 * h);
        }
        a.packed[i] = word;
    } else if (i < L.l[0].tap) {
        int l = 0;
        while (l + 1 < L.n_layers && i >= L.l[l + 1].bias) ++l;
        const int u = (int)(i - L.l[l].bias);
        a.packed[i] = __float_as_uint(u < L.l[l].N ? a.b[l][u] : 0.0f);
    } else {
        int v = 0;
        for (int l = 0; l < L.n_conv; ++l) {
            const Layer& y = L.l[l];
            if (i >= y.tap && i < y.tap + y.kt * 32) v = tap_value(y, (int)(i - y.tap));
            else if (i >= y.pin && i < y.pin + y.mtiles * 16) v = pin_value(y, (int)(i - y.pin));
            else if (i >= y.pout && i < y.pout + y.mtiles * 16) v = pout_value(y, (int)(i - y.pout));
        }
        if (i >= L.st_code) v = st_code_value(L.l[0], L.window, (int)(i - L.st_code));
        else if (i >= L.st_obs) v = st_obs_value(L.l[0], L.window, (int)(i - L.st_obs));
        a.packed[i] = (uint32_t)v;
    }
}

// One conv layer of the group: the implicit GEMM per (env, 16-position M-tile) item, the items dealt to the
// waves; a wave runs IT items at a time, which share each K-slice's tap entries and weight fragments (and give
// the gathers and the MFMAs independent work to overlap).  NT: the layer's N-tiles (cout <= 16 NT).
template <int NT, int IT, typename WP>
__device__ __forceinline__ void conv_layer(const Layer& y, uint32_t* act, WP wsrc, const float* bias, int G, int EW,
                                           int wave, int lane, bool& bad) {
    constexpr float kLo = 1.0f / 2048.0f;
    const int c = lane & 15, g = lane >> 4;
    const int mtiles = y.mtiles, nitems = G * mtiles;
    const uint32_t* tap = wsrc + y.tap;
    for (int it0 = wave; it0 < nitems; it0 += kWaves * IT) {
        const uint32_t* in[IT];
        int e[IT], mt[IT];
        f32x4 acc[IT][NT], acl[IT][NT];
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int item = it0 + u * kWaves < nitems ? it0 + u * kWaves : it0;  // (past the end: it0 again, not stored)
            e[u] = mtiles > 1 ? (int)__umulhi((uint32_t)item, (uint32_t)y.mt_magic) : item;  // item / mtiles
            mt[u] = item - e[u] * mtiles;
            in[u] = act + e[u] * EW + y.in_reg + wsrc[y.pin + 16 * mt[u] + c];  // (rows past the map: position 0)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[u][n] = acl[u][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        for (int t = 0; t < y.kt; ++t) {
            const uint4 o0 = reinterpret_cast<const uint4*>(tap)[8 * t + 2 * g];
            const uint4 o1 = reinterpret_cast<const uint4*>(tap)[8 * t + 2 * g + 1];
            f16x8 wh[NT], wo[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                wh[n] = frag16(wsrc, y.frag_hi + (n * y.kt + t) * 64 + lane);
                wo[n] = frag16(wsrc, y.frag_lo + (n * y.kt + t) * 64 + lane);
            }
#pragma unroll
            for (int u = 0; u < IT; ++u) {
                const uint32_t d[8] = {in[u][o0.x], in[u][o0.y], in[u][o0.z], in[u][o0.w],
                                       in[u][o1.x], in[u][o1.y], in[u][o1.z], in[u][o1.w]};
                f16x8 xh, xl;
                operands(d, xh, xl);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    acc[u][n] = CV_MFMA(xh, wh[n], acc[u][n], 0, 0, 0);
                    acl[u][n] = CV_MFMA(xl, wh[n], acl[u][n], 0, 0, 0);
                    acl[u][n] = CV_MFMA(xh, wo[n], acl[u][n], 0, 0, 0);
                }
            }
        }
        // lane (c, g) holds positions 16 mt + 4 g + i of channel 16 n + c
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            if (it0 + u * kWaves >= nitems) continue;
            const uint4 pv = reinterpret_cast<const uint4*>(wsrc + y.pout)[4 * mt[u] + g];
            const int po[4] = {(int)pv.x, (int)pv.y, (int)pv.z, (int)pv.w};  // (-1: past the map)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int co = 16 * n + c;
                if (co < y.cout) {
                    const float b = bias[co];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (po[i] >= 0) {
                            const float v = fmaxf((acc[u][n][i] + acl[u][n][i] * kLo) + b, 0.0f);
                            act[e[u] * EW + y.out_reg + po[i] + co] = split_word(v, bad);
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------- act ---
// WL: the image (fragments, biases, tap tables) is staged in LDS in front of the env blocks; else it is read
// from global memory (L2).
template <bool WL>
__global__ void __launch_bounds__(kThreads) drl_convnet_act_kernel(ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Layout& L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int G = L.group, EW = L.env_words;
    const int wl_words = WL ? (L.w_words + 3) / 4 * 4 : 0;
    uint32_t* act = lds + wl_words;
    if constexpr (WL)
        for (int i = tid; i < L.w_words; i += kThreads) lds[i] = a.packed[i];
    // (the halos and the dense inputs' K padding stay zero: later passes write the interiors only)
    for (int i = tid; i < G * EW; i += kThreads) act[i] = 0u;
    __syncthreads();
    const uint32_t* wsrc;
    if constexpr (WL) wsrc = lds;
    else wsrc = a.packed;
    constexpr float kLo = 1.0f / 2048.0f;
    bool bad = false;
    const int64_t ngroups = (a.E + G - 1) / G;
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t env0 = grp * G;
        {   // stage the group's windows, split, inside layer 0's halo (envs past E: the last env again); a
            // thread's loads are issued together, then split and stored
            const Layer y0 = L.l[0];
            const int W = L.window;
            uint32_t* dst0 = act + y0.in_reg + (y0.p * y0.pad_side + y0.p) * 6;
            if (L.input == DRL_QNET_INPUT_OBS) {
                const int npair = W * W * 3, total = G * npair;
                constexpr int U = 4;
                for (int i0 = tid; i0 < total; i0 += U * kThreads) {
                    float2 v[U];
                    int e[U], pr[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int idx = i0 + u * kThreads, ic = idx < total ? idx : i0;
                        e[u] = (int)__umulhi((uint32_t)ic, (uint32_t)L.npair_magic);  // ic / npair
                        pr[u] = ic - e[u] * npair;
                        const int64_t env = env0 + e[u] < a.E ? env0 + e[u] : a.E - 1;
                        v[u] = reinterpret_cast<const float2*>(static_cast<const float*>(a.input) + env * a.obs_stride)[pr[u]];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (i0 + u * kThreads < total) {
                            uint32_t* d = dst0 + e[u] * EW + wsrc[L.st_obs + pr[u]];
                            d[0] = split_word(v[u].x, bad);
                            d[1] = split_word(v[u].y, bad);
                        }
                    }
                }
            } else {
                // the policy code (write_code_wave: 4 groups of cpg cells, each padded to cpg8 u16): the
                // channels of drl_code_decode_kernel from (object, air)
                const int cells = W * W, row16 = lay::code_bytes(W) / 2, total = G * cells;
                for (int idx = tid; idx < total; idx += kThreads) {
                    const int e = (int)__umulhi((uint32_t)idx, (uint32_t)L.cells_magic), cl = idx - e * cells;
                    const int64_t env = env0 + e < a.E ? env0 + e : a.E - 1;
                    const uint32_t sd = wsrc[L.st_code + cl];  // the cell's u16 in the row | its map word << 16
                    const uint32_t h = (static_cast<const uint16_t*>(a.input) + env * row16)[sd & 0xffffu];
                    const uint32_t obj = h & 7u, air = h >> 3;
                    uint32_t* d = dst0 + e * EW + (sd >> 16);
                    d[0] = split_word(air ? 1.0f : 0.0f, bad);
                    d[1] = split_word((obj == OBJ_PACKET || (air & 0x80u)) ? 1.0f : 0.0f, bad);
                    d[2] = split_word(obj == OBJ_DROPZONE ? 1.0f : 0.0f, bad);
                    d[3] = split_word(obj == OBJ_STATION ? 1.0f : 0.0f, bad);
                    d[4] = split_word(air ? cv_div100((int)(air & 0x7fu) - 1) : 0.0f, bad);
                    d[5] = split_word(obj == OBJ_SKYSCRAPER ? 1.0f : 0.0f, bad);
                }
            }
        }
        __syncthreads();
        for (int l = 0; l < L.n_layers; ++l) {
            const Layer y = L.l[l];
            const float* bias = reinterpret_cast<const float*>(wsrc + y.bias);
            if (y.conv) {
                if (y.nt == 1) conv_layer<1, 4>(y, act, wsrc, bias, G, EW, wave, lane, bad);
                else conv_layer<2, 2>(y, act, wsrc, bias, G, EW, wave, lane, bad);
            } else {
                // M = the group's envs: lane (c, g) reads env c's row (lanes past the group: env 0's)
                const uint32_t* in = act + (c < G ? c : 0) * EW + y.in_reg;
                const bool head = l + 1 == L.n_layers;
                for (int n = wave; n < y.nt; n += kWaves) {
                    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, acl = acc;
                    for (int t = 0; t < y.kt; ++t) {
                        const uint4 d0 = reinterpret_cast<const uint4*>(in)[8 * t + 2 * g];
                        const uint4 d1 = reinterpret_cast<const uint4*>(in)[8 * t + 2 * g + 1];
                        const uint32_t d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
                        f16x8 xh, xl;
                        operands(d, xh, xl);
                        const f16x8 wh = frag16(wsrc, y.frag_hi + (n * y.kt + t) * 64 + lane);
                        const f16x8 wo = frag16(wsrc, y.frag_lo + (n * y.kt + t) * 64 + lane);
                        acc = CV_MFMA(xh, wh, acc, 0, 0, 0);
                        acl = CV_MFMA(xl, wh, acl, 0, 0, 0);
                        acl = CV_MFMA(xh, wo, acl, 0, 0, 0);
                    }
                    // lane (c, g) holds envs 4 g + i of unit 16 n + c
                    const int u = 16 * n + c;
                    if (u < y.N) {
                        const float b = bias[u];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int e = 4 * g + i;
                            if (e < G) {
                                const float v = (acc[i] + acl[i] * kLo) + b;
                                uint32_t* o = act + e * EW + y.out_reg + u;
                                if (head) *o = __float_as_uint(v);
                                else *o = split_word(fmaxf(v, 0.0f), bad);
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (tid < G && env0 + tid < a.E) {  // the dense acts' epilogue (dronerl_act_common.h)
            const float* qv = reinterpret_cast<const float*>(act + tid * EW + L.q_reg);
            float q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) q[i] = i < L.n_actions ? qv[i] : 0.0f;
            act_epilogue(a, env0 + tid, q, L.n_actions);
        }
        __syncthreads();  // (the next pass rewrites the maps and the Q words)
    }
    flag_qnet_range(a.err, a.packed + L.status, bad, lane);
}

int launch_convnet_pack(const PackArgs& a, hipStream_t s) {
    const int64_t n = a.L.w_words;
    hipLaunchKernelGGL(drl_convnet_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_convnet_act(const ActArgs& a, int num_cus, hipStream_t s) {
    const int G = a.L.group;
    const int64_t ngroups = (a.E + G - 1) / G;
    int per_cu = kLdsMax / a.L.lds_bytes;  // resident workgroups by LDS (8 waves each)
    per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
    int64_t nb = (int64_t)num_cus * per_cu;
    if (nb > ngroups) nb = ngroups;
    const dim3 grid((unsigned)nb), block(kThreads);
    if (a.L.w_lds) hipLaunchKernelGGL(drl_convnet_act_kernel<true>, grid, block, (size_t)a.L.lds_bytes, s, a);
    else hipLaunchKernelGGL(drl_convnet_act_kernel<false>, grid, block, (size_t)a.L.lds_bytes, s, a);
    return (int)hipGetLastError();
}

}  // namespace cv
}  // namespace drl
