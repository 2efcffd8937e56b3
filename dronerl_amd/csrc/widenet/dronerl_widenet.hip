// dronerl_widenet.hip — wide dense Q-networks on the device (include/dronerl.h drl_widenet_*): the pack kernel
// and the forward + epsilon-greedy act for hidden widths up to 256 (run_jax_sweep.py's 256-128-64 net).
//
// Reference: jax_impl/agents/dqn.py:47-63 DenseQNetwork (Dense + ReLU per hidden layer, Dense(n_actions)),
// DQNAgent.act (:132-146); torch_impl/agents/dqn.py:44-82.
//
// Numerics are DRL_QNET_F32's (dronerl_qnet.hip split_f16; the dense tail of convnet/dronerl_convnet.hip): each
// operand v as fp16 hi = fp16(v) and lo = fp16((v - hi) * 2^11); acc += Whi * xhi, acl += Whi * xlo + Wlo * xhi
// on v_mfma_f32_16x16x32_f16; the layer's value is (acc + 2^-11 acl) + bias.  The weights are the A operand and a
// tile of 16 envs the B operand, so the accumulator's column is an env: a lane holds four consecutive units of
// one env, which is one 16-byte LDS store for a hidden layer and dronerl_act_common.h's tile_act for the Q head.
//
// The image (up to ~1.1 MB) does not fit the 160 KB LDS, so the fragments are read from global memory, where
// they stay L2-resident: one 16-byte load per lane per fragment, kPrefetch K-slices ahead, and every fragment a
// wave reads serves all `tiles` env tiles of the workgroup's pass.  A layer's 16-unit tiles are dealt to the 8
// waves, two at a time where there are 16 or more (they share each env tile's unpacked operands).  The activations pass between layers through LDS already split, one 32-bit word per value.  The layout
// arithmetic is dronerl_widenet_layout.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "dronerl_widenet_layout.h"

namespace drl {
namespace wn {

// (the code staging restates the policy code's row geometry)
static_assert(lay::code_cpg(5) == 7 && lay::code_cpg8(5) == 8 && lay::code_cpg(7) == 13 && lay::code_cpg8(7) == 16 &&
              lay::code_cpg(9) == 21 && lay::code_cpg8(9) == 24, "policy code row geometry");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPrefetch = 4;  // K-slices whose fragment loads a wave keeps in flight

#define WN_MFMA __builtin_amdgcn_mfma_f32_16x16x32_f16

__device__ __forceinline__ uint32_t f16_bits(_Float16 h) {
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}

// v as one word: fp16 hi in bits 0-15, fp16 lo in bits 16-31.  `bad`: |v| >= 65520 rounds hi to inf, NaN stays
// NaN (DRL_ERR_QNET_RANGE).
__device__ __forceinline__ uint32_t split_word(float v, bool& bad) {
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)((v - (float)h) * 2048.0f);
    bad |= !(__builtin_fabsf(v) < 65520.0f);
    return f16_bits(h) | (f16_bits(l) << 16);
}

// 8 split words -> the hi and the lo MFMA operand
__device__ __forceinline__ void operands(const uint4& d0, const uint4& d1, f16x8& hi, f16x8& lo) {
    const uint32_t d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    uint32_t h[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        h[p] = (d[2 * p] & 0xffffu) | (d[2 * p + 1] << 16);
        l[p] = (d[2 * p] >> 16) | (d[2 * p + 1] & 0xffff0000u);
    }
    __builtin_memcpy(&hi, h, 16);
    __builtin_memcpy(&lo, l, 16);
}

__device__ __forceinline__ f16x8 frag16(const uint4* p) {
    const uint4 v = *p;
    f16x8 f;
    __builtin_memcpy(&f, &v, 16);
    return f;
}

// drl_obs's charge channel (dronerl_kernels.hip div100: c / 100 correctly rounded)
__device__ __forceinline__ float wn_div100(int c) {
    const float x = (float)c;
    const float r = 0.01f;
    const float q = x * r;
    const float e = __fmaf_rn(-q, 100.0f, x);
    return __fmaf_rn(e, r, q);
}

// ------------------------------------------------------------------ pack ---
// One thread per 32-bit word of the image before the status vector: two fp16 fragment elements (hi or lo pieces
// of the weights frag_elem names, zero in the K and unit padding) or a bias (zero past the layer's units).
__global__ void __launch_bounds__(256) drl_widenet_pack_kernel(PackArgs a) {
    const Layout& L = a.L;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.w_words) return;
    if (i < L.frag_words) {
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
            int unit, k;
            frag_elem(y, e0 + h, &unit, &k);
            const float w = unit < y.out && k < y.in ? a.w[l][(int64_t)unit * y.in + k] : 0.0f;
            if (!lo && !(__builtin_fabsf(w) < 65504.0f))
                atomicOr(reinterpret_cast<int32_t*>(a.packed + L.status), DRL_ERR_QNET_RANGE);
            const _Float16 hi = (_Float16)w;
            word |= f16_bits(lo ? (_Float16)((w - (float)hi) * 2048.0f) : hi) << (16 * h);
        }
        a.packed[i] = word;
    } else {
        int l = 0;
        while (l + 1 < L.n_layers && i >= L.l[l + 1].bias) ++l;
        const int u = (int)(i - L.l[l].bias);
        a.packed[i] = __float_as_uint(u < L.l[l].out ? a.b[l][u] : 0.0f);
    }
}

// ------------------------------------------------------------------- act ---
// One layer of the pass: NT 16-unit tiles by TW env tiles per wave iteration (y.nt % NT == 0); the NT tiles share
// each env tile's operands, read from LDS and unpacked once.  in / out: the stages' first words in LDS, rs_in /
// rs_out their row strides.  HEAD: the Q head (one tile): the epilogue instead of the store.
template <int TW, int NT, bool HEAD>
__device__ __forceinline__ void wide_layer(const ActArgs& a, const Layer& y, const uint32_t* in, int rs_in, uint32_t* out,
                                           int rs_out, int64_t env0, int wave, int lane, bool& bad) {
    constexpr float kLo = 1.0f / 2048.0f;
    const int c = lane & 15, g = lane >> 4;
    const int kt = y.kt;
    const uint4* img = reinterpret_cast<const uint4*>(a.packed);
    for (int n0 = NT * wave; n0 < y.nt; n0 += NT * kWaves) {
        // tiles n0 .. n0 + NT - 1: their fragments of a K-slice are kt * 64 vectors apart
        const uint4* fh = img + y.frag_hi + (int64_t)n0 * kt * 64 + lane;
        const uint4* fl = img + y.frag_lo + (int64_t)n0 * kt * 64 + lane;
        f16x8 wh[kPrefetch][NT], wo[kPrefetch][NT];
#pragma unroll
        for (int p = 0; p < kPrefetch; ++p) {
            const int t = p < kt ? p : kt - 1;  // (past the layer: the last slice again, not used)
#pragma unroll
            for (int v = 0; v < NT; ++v) {
                wh[p][v] = frag16(fh + (v * kt + t) * 64);
                wo[p][v] = frag16(fl + (v * kt + t) * 64);
            }
        }
        f32x4 acc[NT][TW], acl[NT][TW];
#pragma unroll
        for (int v = 0; v < NT; ++v)
#pragma unroll
            for (int u = 0; u < TW; ++u) acc[v][u] = acl[v][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int t0 = 0; t0 < kt; t0 += kPrefetch) {
#pragma unroll
            for (int p = 0; p < kPrefetch; ++p) {
                const int t = t0 + p;
                if (t < kt) {
#pragma unroll
                    for (int u = 0; u < TW; ++u) {
                        // env 16 u + c's inputs 32 t + 8 g .. + 7
                        const uint4* row = reinterpret_cast<const uint4*>(in + (16 * u + c) * rs_in + 32 * t + 8 * g);
                        f16x8 xh, xl;
                        operands(row[0], row[1], xh, xl);
#pragma unroll
                        for (int v = 0; v < NT; ++v) {
                            acc[v][u] = WN_MFMA(wh[p][v], xh, acc[v][u], 0, 0, 0);
                            acl[v][u] = WN_MFMA(wh[p][v], xl, acl[v][u], 0, 0, 0);
                            acl[v][u] = WN_MFMA(wo[p][v], xh, acl[v][u], 0, 0, 0);
                        }
                    }
                }
                if (t + kPrefetch < kt) {
#pragma unroll
                    for (int v = 0; v < NT; ++v) {
                        wh[p][v] = frag16(fh + (v * kt + t + kPrefetch) * 64);
                        wo[p][v] = frag16(fl + (v * kt + t + kPrefetch) * 64);
                    }
                }
            }
        }
        // lane (c, g) holds units 16 n + 4 g + i of env 16 u + c
#pragma unroll
        for (int v = 0; v < NT; ++v) {
            const int n = n0 + v;
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.packed + y.bias) + 16 * n + 4 * g);
            const float bi[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int u = 0; u < TW; ++u) {
                if constexpr (HEAD) {
                    tile_act(a, env0 + 16 * u + c, lane, [&](int i) { return (acc[v][u][i] + acl[v][u][i] * kLo) + bi[i]; });
                } else {
                    uint4 o;
                    o.x = split_word(fmaxf((acc[v][u][0] + acl[v][u][0] * kLo) + bi[0], 0.0f), bad);
                    o.y = split_word(fmaxf((acc[v][u][1] + acl[v][u][1] * kLo) + bi[1], 0.0f), bad);
                    o.z = split_word(fmaxf((acc[v][u][2] + acl[v][u][2] * kLo) + bi[2], 0.0f), bad);
                    o.w = split_word(fmaxf((acc[v][u][3] + acl[v][u][3] * kLo) + bi[3], 0.0f), bad);
                    *reinterpret_cast<uint4*>(out + (16 * u + c) * rs_out + 16 * n + 4 * g) = o;
                }
            }
        }
    }
}

// TW: the plan's tiles per pass (Layout::tiles).
template <int TW>
__global__ void __launch_bounds__(kThreads) drl_widenet_act_kernel(ActArgs args) {
    (void)args;  // (read in place: a layer index into a by-value copy would put the layout in scratch)
    const ActArgs& a = *(const ActArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Layout& L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int G = 16 * TW;
    bool bad = false;
    const int64_t ngroups = (a.E + G - 1) / G;
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t env0 = grp * G;
        {   // stage the group's inputs, split (envs past E: the last env again); every column of stage 0's K-slices
            // is written, the pads with zeros (a later layer's outputs shared the region)
            uint32_t* s0 = lds + L.region[0];
            const int rs0 = L.rs[0], in = L.l[0].in;
            if (L.input == DRL_QNET_INPUT_OBS) {
                const int npair = 16 * L.l[0].kt, total = G * npair;
                constexpr int U = 4;
                for (int i0 = tid; i0 < total; i0 += U * kThreads) {
                    float2 v[U];
                    int e[U], pr[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int idx = i0 + u * kThreads, ic = idx < total ? idx : i0;
                        e[u] = (int)__umulhi((uint32_t)ic, (uint32_t)L.pairs_magic);  // ic / npair
                        pr[u] = ic - e[u] * npair;
                        const int64_t env = env0 + e[u] < a.E ? env0 + e[u] : a.E - 1;
                        v[u] = make_float2(0.0f, 0.0f);
                        if (2 * pr[u] < in)
                            v[u] = reinterpret_cast<const float2*>(static_cast<const float*>(a.input) + env * a.obs_stride)[pr[u]];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (i0 + u * kThreads < total) {
                            uint2 w;
                            w.x = split_word(v[u].x, bad);
                            w.y = split_word(v[u].y, bad);
                            *reinterpret_cast<uint2*>(s0 + e[u] * rs0 + 2 * pr[u]) = w;
                        }
                    }
                }
            } else {
                // the policy code (write_code_wave: 4 groups of cpg cells, each padded to cpg8 u16): the channels
                // of drl_code_decode_kernel from (object, air)
                const int W = L.code_w, cells = W * W, row16 = lay::code_bytes(W) / 2, total = G * cells;
                const int cpg = lay::code_cpg(W), cpg8 = lay::code_cpg8(W);
                for (int idx = tid; idx < total; idx += kThreads) {
                    const int e = (int)__umulhi((uint32_t)idx, (uint32_t)L.cells_magic), cl = idx - e * cells;
                    const int64_t env = env0 + e < a.E ? env0 + e : a.E - 1;
                    const int grp4 = (cl >= cpg) + (cl >= 2 * cpg) + (cl >= 3 * cpg);  // cl / cpg
                    const uint32_t h = (static_cast<const uint16_t*>(a.input) + env * row16)[grp4 * cpg8 + (cl - grp4 * cpg)];
                    const uint32_t obj = h & 7u, air = h >> 3;
                    uint32_t* d = s0 + e * rs0 + cl * 6;
                    uint2 w;
                    w.x = split_word(air ? 1.0f : 0.0f, bad);
                    w.y = split_word((obj == OBJ_PACKET || (air & 0x80u)) ? 1.0f : 0.0f, bad);
                    *reinterpret_cast<uint2*>(d) = w;
                    w.x = split_word(obj == OBJ_DROPZONE ? 1.0f : 0.0f, bad);
                    w.y = split_word(obj == OBJ_STATION ? 1.0f : 0.0f, bad);
                    *reinterpret_cast<uint2*>(d + 2) = w;
                    w.x = split_word(air ? wn_div100((int)(air & 0x7fu) - 1) : 0.0f, bad);
                    w.y = split_word(obj == OBJ_SKYSCRAPER ? 1.0f : 0.0f, bad);
                    *reinterpret_cast<uint2*>(d + 4) = w;
                }
                const int npad = 32 * L.l[0].kt - in;
                for (int idx = tid; idx < G * npad; idx += kThreads) {
                    const int e = idx / npad;
                    s0[e * rs0 + in + (idx - e * npad)] = 0u;
                }
            }
        }
        __syncthreads();
        for (int l = 0; l < L.n_layers; ++l) {
            const Layer& y = L.l[l];
            const uint32_t* in = lds + L.region[l & 1];
            if (l + 1 == L.n_layers) {
                wide_layer<TW, 1, true>(a, y, in, L.rs[l], nullptr, 0, env0, wave, lane, bad);
            } else if (y.nt >= 2 * kWaves) {  // (a hidden layer's tile count is even) two tiles per wave at a time
                wide_layer<TW, 2, false>(a, y, in, L.rs[l], lds + L.region[(l + 1) & 1], L.rs[l + 1], env0, wave, lane, bad);
            } else {
                wide_layer<TW, 1, false>(a, y, in, L.rs[l], lds + L.region[(l + 1) & 1], L.rs[l + 1], env0, wave, lane, bad);
            }
            __syncthreads();  // (the next layer reads the outputs; the next pass rewrites the inputs)
        }
    }
    flag_qnet_range(a.err, a.packed + L.status, bad, lane);
}

int launch_widenet_pack(const PackArgs& a, hipStream_t s) {
    const int64_t n = a.L.w_words;
    hipLaunchKernelGGL(drl_widenet_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_widenet_act(const ActArgs& a, int num_cus, hipStream_t s) {
    const dim3 grid((unsigned)act_grid(a.L, a.E, num_cus)), block(kThreads);
    const size_t lds = (size_t)a.L.lds_bytes;
    if (a.L.tiles == 4) hipLaunchKernelGGL(drl_widenet_act_kernel<4>, grid, block, lds, s, a);
    else if (a.L.tiles == 2) hipLaunchKernelGGL(drl_widenet_act_kernel<2>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(drl_widenet_act_kernel<1>, grid, block, lds, s, a);
    return (int)hipGetLastError();
}

}  // namespace wn
}  // namespace drl
