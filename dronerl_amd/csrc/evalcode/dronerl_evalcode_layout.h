// dronerl_evalcode_layout.h — launch geometry and argument blocks of the multi-agent evaluation kernels
// (dronerl_evalcode.hip; include/dronerl.h drl_obs_code_all / drl_score_add), shared with their C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dronerl_internal.h"

namespace drl {
namespace ec {

// DRL_EC_TARGET_CELLS / DRL_EC_MAX_EPW: tuning knobs for A/B builds (the window cells a wave aims to build, which
// sets its envs per wave, and their cap)
#ifndef DRL_EC_TARGET_CELLS
#define DRL_EC_TARGET_CELLS 1024
#endif
#ifndef DRL_EC_MAX_EPW
#define DRL_EC_MAX_EPW 8
#endif
constexpr int kLdsBudget = 64 * 1024;  // dynamic LDS a one-wave workgroup may ask for
constexpr int kTargetCells = DRL_EC_TARGET_CELLS;
constexpr int kMaxEnvsPerWave = DRL_EC_MAX_EPW;

// One wave (= one workgroup) builds the rows of `epw` consecutive envs.  Its LDS, every region a 16-B multiple:
//   ground  u8  [epw][pstride]        the envs' packed nibble rows, as they lie in HBM (one contiguous copy)
//   rec     u32 [epw][N]              the drone records by drone index (HBM holds them in dict order)
//   rows    u16 [N][epw][4 * cpg8]    the code rows, drone-major like the output (one contiguous run per drone)
struct Geom {
    int side, N, R, W, cells, cpg, cpg8, pstride, epw;
    int off_rec, off_rows, lds_bytes;  // byte offsets of rec / rows in the wave's LDS, and its size
    FastDiv div_w, div_cpg, div_n;
};

inline int lds_bytes_for(int epw, int pstride, int N, int cpg8) {
    return epw * pstride + lay::r16(epw * N * 4) + epw * N * 8 * cpg8;
}

// Geometry of a validated params set (side <= DRL_MAX_SIDE, N <= DRL_MAX_DRONES, radius <= DRL_MAX_RADIUS: one
// env always fits kLdsBudget -- 8192 + 256 + 64 * 640 B at the limits).
inline Geom geom_of(int side, int N, int R) {
    Geom g;
    g.side = side;
    g.N = N;
    g.R = R;
    g.W = 2 * R + 1;
    g.cells = g.W * g.W;
    g.cpg = lay::code_cpg(g.W);
    g.cpg8 = lay::code_cpg8(g.W);
    g.pstride = lay::pstride(side);
    int epw = kTargetCells / (N * g.cells);
    epw = epw < 1 ? 1 : (epw > kMaxEnvsPerWave ? kMaxEnvsPerWave : epw);
    while (epw > 1 && lds_bytes_for(epw, g.pstride, N, g.cpg8) > kLdsBudget) --epw;
    g.epw = epw;
    g.off_rec = epw * g.pstride;
    g.off_rows = g.off_rec + lay::r16(epw * N * 4);
    g.lds_bytes = lds_bytes_for(epw, g.pstride, N, g.cpg8);
    g.div_w = make_fastdiv((uint32_t)g.W);
    g.div_cpg = make_fastdiv((uint32_t)g.cpg);
    g.div_n = make_fastdiv((uint32_t)N);
    return g;
}

struct CodeAllArgs {
    Geom g;
    int64_t E;
    const uint8_t* ground;
    const uint32_t* drones;
    uint4* codes;
};

struct ScoreArgs {
    const float* rewards;
    double* scores;
    int64_t n;  // E * n_drones
    double v_crash, v_charge, v_pickup, v_delivery;
    float f_crash, f_charge, f_pickup, f_delivery;
};

hipError_t launch_obs_code_all(const CodeAllArgs& a, hipStream_t s);
hipError_t launch_score_add(const ScoreArgs& a, hipStream_t s);

}  // namespace ec
}  // namespace drl
