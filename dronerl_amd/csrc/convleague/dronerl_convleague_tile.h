// dronerl_convleague_tile.h — the per-layer arithmetic of a tile of T rows in LDS, shared by the two conv acts
// that tile their rows (convleague/dronerl_convleague.hip: a tile is T envs of one drone; convselfplay/
// dronerl_convselfplay.hip: T rows of a learner's team).  Device only: included by the .hip units after their
// `#pragma clang fp contract(off)`.  tile_forward works on LDS rows alone: which global row a tile row was decoded
// from, and where its action goes, is each kernel's own business.  The arithmetic of a row is cl::cl_forward's
// (convlearn/dronerl_convlearn_rows.h) bit for bit; the tiling decides which thread does a sum, never its order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"
#include "../dronerl_act_common.h"
#include "../dronerl_learn_common.h"
#include "dronerl_convleague_layout.h"

// every product and sum rounds on its own (no FMA contraction), as in the learners
#pragma clang fp contract(off)

namespace drl {
namespace cvl {

namespace {

// what dq_input reads of its argument block
struct CodeRows {
    int64_t row_words;
    int32_t code_w;
};

// what the act epilogue reads of its argument block (dronerl_act_common.h)
struct Epilogue {
    uint64_t seed, step;
    int64_t env_offset;
    const float* eps_ptr;
    float epsilon;
    int32_t* actions;
    int64_t action_stride;
    float* q;
};

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// Layer l of the tile's T rows (cl_forward's sums, T envs at a time).  `rows` is the tile's LDS; row r starts at
// word r * S.  Rows past the tile's envs hold 0.0 inputs; their outputs are computed and never leave LDS.
template <int T>
__device__ __forceinline__ void tile_forward(const cl::Plan& P, const ActPlan& A, int l, const float* __restrict__ W,
                                             float* rows) {
    const cl::LLayer& q = P.l[l];
    const int tid = threadIdx.x, nt = blockDim.x, S = A.row_words;
    const float* w = W + q.woff;
    const float* bias = W + q.boff;
    const float* x = rows + in_word(A, l);
    float* out = rows + A.out[l];
    const bool relu = l + 1 < P.n_layers;
    if (q.conv) {
        const int os = q.out_side, is = q.in_side, hw = os * os, k = q.k;
        for (int e = tid; e < q.n_out; e += nt) {
            const int co = e / hw, pos = e - co * hw, oy = pos / os, ox = pos - oy * os;
            const float* wc = w + (int64_t)co * q.K;
            // the taps inside the map: ky in [ky0, ky1), kx in [kx0, kx1) (cl_forward skips the others)
            const int y0 = oy * q.s - q.p, x0 = ox * q.s - q.p;
            const int ky0 = imax(0, -y0), ky1 = imin(k, is - y0), kx0 = imax(0, -x0), kx1 = imin(k, is - x0);
            float z[T];
#pragma unroll
            for (int t = 0; t < T; ++t) z[t] = 0.0f;
            for (int ci = 0; ci < q.cin; ++ci)
                for (int ky = ky0; ky < ky1; ++ky) {
                    const int iy = y0 + ky;
                    for (int kx = kx0; kx < kx1; ++kx) {
                        const int ix = x0 + kx;
                        // layer 0 reads the observation's [y][x][c]; later layers the previous [c][y][x]
                        const int xi = l == 0 ? (iy * is + ix) * 6 + ci : (ci * is + iy) * is + ix;
                        const float wv = wc[(ci * k + ky) * k + kx];
#pragma unroll
                        for (int t = 0; t < T; ++t) z[t] = z[t] + wv * x[t * S + xi];
                    }
                }
            const float b = bias[co];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float v = z[t] + b;
                out[t * S + e] = relu ? (v > 0.0f ? v : 0.0f) : v;
            }
        }
    } else {
        // one wave per unit: lane c sums k = c (mod 64) in k order for each env, then a fixed xor tree
        const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
        for (int j = wave; j < q.n_out; j += nw) {
            const float* wj = w + (int64_t)j * q.K;
            float s[T];
#pragma unroll
            for (int t = 0; t < T; ++t) s[t] = 0.0f;
            for (int kk = lane; kk < q.K; kk += 64) {
                const float wv = wj[kk];
#pragma unroll
                for (int t = 0; t < T; ++t) s[t] = s[t] + wv * x[t * S + kk];
            }
            for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
                for (int t = 0; t < T; ++t) s[t] = s[t] + __shfl_xor(s[t], m);
            }
            const float b = bias[j];
            if (lane == 0) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float v = s[t] + b;
                    out[t * S + j] = relu ? (v > 0.0f ? v : 0.0f) : v;
                }
            }
        }
    }
}

}  // namespace

}  // namespace cvl
}  // namespace drl
