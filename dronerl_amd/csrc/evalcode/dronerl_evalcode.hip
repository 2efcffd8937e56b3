// dronerl_evalcode.hip — the multi-agent evaluator's kernels (include/dronerl.h drl_obs_code_all, drl_score_add;
// dronerl_amd/evaluator.py).
//
//  drl_obs_code_all_kernel   the policy code of EVERY drone index of every env, u8 [n_drones][E][code bytes]:
//                            row (d, e) is what drl_obs_code writes for drone index 0, centred on drone index d
//                            (write_obs_wave<CODE> in dronerl_kernels.hip: u16 per cell = object | air << 3,
//                            air = (charge + 1) | carry << 7 of the drone standing there, walls as skyscrapers,
//                            four groups of cpg cells padded with zero codes to cpg8).
//  drl_score_add_kernel      scores[e][d] += the Python double of the step's f32 reward (compat._py_reward).
//
// Geometry of the code kernel (dronerl_evalcode_layout.h): one wave per workgroup, `epw` consecutive envs per
// wave.  The wave copies the envs' packed ground rows (contiguous in HBM) into LDS with 16-B loads, files the
// drone records by drone index, and builds the rows in an LDS image laid out like the output:
//   1. every (env, drone, window cell): the ground nibble under the cell (or DRL_SKYSCRAPER outside the grid); a
//      lane keeps its cell and walks the rows, so the cell's arithmetic is done once and a row costs a few VALU ops
//   2. every (env, drone d, drone d'): d' ORs its air byte into d's row where it stands inside d's window --
//      N * N tests instead of a side * side air image per env (drl_obs_kernel's `paint`), whose zeroing alone
//      would cost more than the rows at large sides
//   3. each drone's epw rows, one contiguous run of the output, leave as 16-B stores.
// No global atomics, no waiting on other workgroups; every global index is bounded by E and n_drones.
#include "dronerl_evalcode_layout.h"

namespace drl {
namespace ec {
namespace {

__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) { return f.one ? n : __umulhi(n, f.m); }

__global__ void __launch_bounds__(64) drl_obs_code_all_kernel(CodeAllArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Geom& g = a.g;
    const int lane = (int)threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * g.epw;
    if (e0 >= a.E) return;
    const int ne = (int)(a.E - e0 < (int64_t)g.epw ? a.E - e0 : (int64_t)g.epw);
    const int N = g.N, W = g.W, R = g.R, G = g.side;
    uint8_t* gl = lds;
    uint32_t* rec = reinterpret_cast<uint32_t*>(lds + g.off_rec);
    uint16_t* rows = reinterpret_cast<uint16_t*>(lds + g.off_rows);
    const int row_u16 = 4 * g.cpg8;  // u16 per code row
    const int VR = g.cpg8 / 2;       // 16-B vectors per code row

    // stage: ground rows (ne * pstride bytes, contiguous), zeroed records and rows, then the records by index
    // (a wave's first 64 records -- all of them unless epw * N > 64 -- are loaded with the ground, one round trip)
    const int nrec = ne * N;
    const uint32_t r_first = lane < nrec ? a.drones[e0 * N + lane] : 0u;
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.ground + e0 * g.pstride);
        uint4* dst = reinterpret_cast<uint4*>(gl);
        for (int v = lane; v < ne * (g.pstride / 16); v += 64) dst[v] = src[v];
        uint4* z = reinterpret_cast<uint4*>(lds + g.off_rec);
        const int nz = (g.lds_bytes - g.off_rec) / 16;
        for (int v = lane; v < nz; v += 64) z[v] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    for (int i = lane; i < nrec; i += 64) {
        const uint32_t r = i < 64 ? r_first : a.drones[e0 * N + i];
        const int el = (int)fdiv((uint32_t)i, g.div_n);
        const int idx = (int)(r >> 25);
        if (idx < N) rec[el * N + idx] = r;  // (an index >= N is no valid state: its record is left out)
    }
    __syncthreads();

    // 1. objects: a lane keeps one window cell (c = lane, then lane + 64, ...: its offsets from the centre and its
    // slot in a row are worked out once) and walks the wave's rows, whose records are wave-uniform
    for (uint32_t c = (uint32_t)lane; c < (uint32_t)g.cells; c += 64) {
        const uint32_t wy = fdiv(c, g.div_w), wx = c - wy * (uint32_t)W;
        const int oy = (int)wy - R, ox = (int)wx - R;
        const uint32_t slot = fdiv(c, g.div_cpg) * (uint32_t)(g.cpg8 - g.cpg) + c;
        int el = 0, d = 0;
        for (int r = 0; r < nrec; ++r) {  // r = el * N + d
            const uint32_t rc = rec[r];
            const int y = (int)(rc & 255u) + oy, x = (int)((rc >> 8) & 255u) + ox;
            uint32_t obj = (uint32_t)OBJ_SKYSCRAPER;
            if ((unsigned)y < (unsigned)G && (unsigned)x < (unsigned)G) {
                const int k = y * G + x;
                obj = (gl[el * g.pstride + (k >> 1)] >> (4 * (k & 1))) & 15u;
            }
            rows[(d * g.epw + el) * row_u16 + slot] = (uint16_t)obj;
            if (++d == N) {
                d = 0;
                ++el;
            }
        }
    }
    __syncthreads();

    // 2. air bytes: drone d2 inside drone d's window (d2 == d: the centre cell)
    const uint32_t n_pair = (uint32_t)(ne * N) * (uint32_t)N;
    for (uint32_t q = (uint32_t)lane; q < n_pair; q += 64) {
        const uint32_t r = fdiv(q, g.div_n), d2 = q - r * (uint32_t)N;
        const uint32_t el = fdiv(r, g.div_n), d = r - el * (uint32_t)N;
        const uint32_t rc = rec[el * N + d], r2 = rec[el * N + d2];
        const int dy = (int)(r2 & 255u) - (int)(rc & 255u) + R;
        const int dx = (int)((r2 >> 8) & 255u) - (int)((rc >> 8) & 255u) + R;
        if ((unsigned)dy < (unsigned)W && (unsigned)dx < (unsigned)W) {
            const uint32_t c = (uint32_t)(dy * W + dx), grp = fdiv(c, g.div_cpg);
            const uint32_t air = ((((r2 >> 16) & 255u) + 1u) | (((r2 >> 24) & 1u) << 7)) & 255u;
            uint16_t* h = &rows[(d * g.epw + el) * row_u16 + grp * (uint32_t)(g.cpg8 - g.cpg) + c];
            *h = (uint16_t)((*h & 15u) | (air << 3));
        }
    }
    __syncthreads();

    // 3. drone d's ne rows: one contiguous run of ne * VR vectors at row (d, e0)
    const uint4* rv = reinterpret_cast<const uint4*>(rows);
    const uint32_t nv = (uint32_t)(ne * VR), n_vec = nv * (uint32_t)N;
    for (uint32_t t = (uint32_t)lane; t < n_vec; t += 64) {
        const uint32_t d = t / nv, j = t - d * nv;
        a.codes[((int64_t)d * a.E + e0) * VR + j] = rv[d * (uint32_t)(g.epw * VR) + j];
    }
}

// One thread per (env, drone): the first configured reward whose f32 rounding equals the f32 reward gives its
// double (crash, charge, pickup, delivery: compat._py_reward's order), a zero reward 0, anything else widens.
__global__ void __launch_bounds__(256) drl_score_add_kernel(ScoreArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const float r = a.rewards[i];
    double v;
    if (r == a.f_crash) v = a.v_crash;
    else if (r == a.f_charge) v = a.v_charge;
    else if (r == a.f_pickup) v = a.v_pickup;
    else if (r == a.f_delivery) v = a.v_delivery;
    else if (r == 0.0f) v = 0.0;
    else v = (double)r;
    a.scores[i] += v;
}

}  // namespace

hipError_t launch_obs_code_all(const CodeAllArgs& a, hipStream_t s) {
    const int64_t blocks = (a.E + a.g.epw - 1) / a.g.epw;
    hipLaunchKernelGGL(drl_obs_code_all_kernel, dim3((unsigned)blocks), dim3(64), (size_t)a.g.lds_bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_score_add(const ScoreArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(drl_score_add_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ec
}  // namespace drl
