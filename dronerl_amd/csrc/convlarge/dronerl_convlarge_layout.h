// dronerl_convlarge_layout.h — the agent block of the conv DQN learner at replay batches up to 4096
// (include/dronerl.h drl_convnet_dqn_large_*).  The parameter sets, the counters, the parameter map and a row's
// working set are the conv learner's (convlearn/dronerl_convlearn_layout.h: the same drl_convnet_dqn_layout, the
// same per-row words); the scratch is larger: the rows' squared errors [4096], the rows [batch], and every
// chunk's partial gradient of every parameter [ceil(batch / 64)][n_params].  Plain C++ (no HIP): the host API,
// the kernels and tests/native/convlarge_layout_check.cpp share it.
#ifndef DRONERL_CONVLARGE_LAYOUT_H
#define DRONERL_CONVLARGE_LAYOUT_H

#include <stdint.h>

#include "../convlearn/dronerl_convlearn_layout.h"

namespace drl {
namespace cg {

constexpr int kMaxBatch = DRL_CONVNET_DQN_LARGE_MAX_BATCH;
constexpr int kChunkRows = 64;                      // rows of one chunk: the unit of the fixed reduction order
constexpr int kMaxChunks = kMaxBatch / kChunkRows;  // 64: the counters kernel gives a chunk's loss sum a thread
// the rows kernel's workgroup (one per sampled row): 256 threads; at batches up to kRowsWideBatch a multiple of
// 256 up to kRowsThreadsMax, by the widest layer (Tiles::rows_threads).  A row's arithmetic does not depend on the
// count.  Measured on the sweep's conv net: up to about two rows per compute unit the call waits for one row's
// chain of layers, which 1024 threads cut from 1.11 ms to 0.45 ms (batch 256); with every compute unit full,
// the wide workgroup is the slower one (5.2 against 3.8 ms at batch 4096).
constexpr int kRowsThreadsMax = 1024;
constexpr int kRowsWideBatch = 512;
constexpr int kThreads = 256;                       // the gradient and update kernels' workgroup
// the dense-layer partials' tile: a workgroup takes a chunk's rows by kTileUnits units by kTileCols columns of
// [W_l | b_l]; a thread keeps kUnitsPerThread units of one column in registers
constexpr int kTileCols = 64;
constexpr int kUnitsPerThread = 8;
constexpr int kTileUnits = (kThreads / kTileCols) * kUnitsPerThread;  // 32
constexpr int kConvWaves = kThreads / 64;  // conv parameter groups per workgroup of the conv partials' kernel
constexpr int kMaxKernel = 5;              // drl_convnet_desc's kernel_size limit: a group's k x k accumulators
static_assert(kMaxBatch % kChunkRows == 0 && kMaxChunks <= 64, "a chunk's loss sum per thread of one wave");

// What the chain adds to the conv learner's plan: the chunks, the dense partials' tiles, the partials' place.
struct Tiles {
    int32_t chunks;       // ceil(batch / 64)
    int32_t dense_tiles;  // workgroups per chunk of the dense partials' kernel: the sum of the dense layers' tiles
    int32_t tile_base[cl::kMaxLayers + 1];  // layer l's first tile (a conv layer has none); [n_layers]: the total
    int32_t col_tiles[cl::kMaxLayers];      // layer l's tiles along [W | b]'s columns (K + 1 of them)
    int64_t part_off;     // words from the scratch's start: the partials [chunks][n_params rounded up to 4]
    // the conv partials' kernel gives a wave a parameter group: the k x k weights of one (layer, co, ci), or the
    // bias of one (layer, co); conv layer l has cout * (cin + 1) groups, from group_base[l]
    int32_t conv_groups;
    int32_t group_base[cv::kMaxConv + 1];
    int32_t rows_threads;  // the rows kernel's workgroup
};

struct Plan {
    cl::Plan c;  // the net, the row's words and the parameter map; c.batch is this learner's (1..4096)
    Tiles t;
};

// tiles of a dense layer along its columns (the bias is column K) and its units
inline int32_t col_tiles(const cl::LLayer& q) { return (q.K + 1 + kTileCols - 1) / kTileCols; }
inline int32_t unit_tiles(const cl::LLayer& q) { return (q.n_out + kTileUnits - 1) / kTileUnits; }

// Validate a description and a batch and lay the agent block out.  Returns nullptr, or the message for
// drl_last_error.  (The net's and the row's limits are checked by the conv learner's plan at batch 1.)
inline const char* plan(const drl_convnet_desc* d, int32_t batch, Plan* P) {
    *P = Plan{};
    if (const char* msg = cl::plan(d, 1, &P->c)) return msg;
    if (batch < 1 || batch > kMaxBatch) return "batch must be in [1, 4096] (DRL_CONVNET_DQN_LARGE_MAX_BATCH)";
    cl::Plan& C = P->c;
    Tiles& T = P->t;
    C.batch = batch;
    T.chunks = (batch + kChunkRows - 1) / kChunkRows;
    int32_t t = 0;
    for (int l = 0; l < C.n_layers; ++l) {
        T.tile_base[l] = t;
        if (C.l[l].conv) continue;
        T.col_tiles[l] = col_tiles(C.l[l]);
        t += T.col_tiles[l] * unit_tiles(C.l[l]);
    }
    T.tile_base[C.n_layers] = t;
    T.dense_tiles = t;
    int32_t groups = 0, widest = 0;
    for (int l = 0; l < C.n_layers; ++l) {
        if (l < C.n_conv) {
            if (C.l[l].k > kMaxKernel) return "kernel_size must be in [1, 5]";
            T.group_base[l] = groups;
            groups += C.l[l].cout * (C.l[l].cin + 1);
        }
        widest = C.l[l].n_out > widest ? C.l[l].n_out : widest;
    }
    T.group_base[C.n_conv] = groups;
    T.conv_groups = groups;
    T.rows_threads = batch <= kRowsWideBatch ? (widest + 255) / 256 * 256 : 256;
    T.rows_threads = T.rows_threads > kRowsThreadsMax ? kRowsThreadsMax : T.rows_threads;
    C.sq_off = 0;
    C.rows_off = kMaxBatch;
    T.part_off = C.rows_off + (int64_t)batch * C.row_words;
    C.scratch_words = T.part_off + (int64_t)T.chunks * cl::r4(C.n_params);
    C.pub.bytes = C.pub.scratch_off + C.scratch_words * 4;
    return nullptr;
}

// word (from the scratch's start) of chunk c's partial gradient of parameter i
DRL_CV_HD int64_t part_word(const cl::Plan& C, const Tiles& T, int c, int64_t i) {
    return T.part_off + (int64_t)c * ((C.n_params + 3) / 4 * 4) + i;
}

// The dense partials' kernel, tile t of a chunk: its layer, and the first column and unit it takes.
struct TileRef {
    int32_t layer, k0, j0;
};

DRL_CV_HD TileRef tile_locate(const cl::Plan& C, const Tiles& T, int t) {
    int l = C.n_conv;
    while (l + 1 < C.n_layers && t >= T.tile_base[l + 1]) ++l;
    const int e = t - T.tile_base[l], ut = e / T.col_tiles[l];
    return TileRef{l, (e - ut * T.col_tiles[l]) * kTileCols, ut * kTileUnits};
}

// The conv partials' kernel, group g: its layer and output channel, and its input channel (== cin: the bias).
struct GroupRef {
    int32_t layer, co, ci;
};

DRL_CV_HD GroupRef group_locate(const cl::Plan& C, const Tiles& T, int g) {
    int l = 0;
    while (l + 1 < C.n_conv && g >= T.group_base[l + 1]) ++l;
    const int e = g - T.group_base[l], per = C.l[l].cin + 1, co = e / per;
    return GroupRef{l, co, e - co * per};
}

// ---- kernel arguments (dronerl_convlarge.hip; launched by dronerl_convlarge_api.cpp) ------------------------
struct LearnArgs {
    cl::LearnArgs a;  // (a.P is the plan's c; the fields dronerl_learn_common.h's functions read)
    Tiles t;
};

// (hipError_t values) one learner step's launches, in stream order
int launch_convlarge_train(const LearnArgs& a, hipStream_t s);
// ... and that chain behind its rows kernel (the chunk partials with a sample, the update, the counters), which
// the prioritized chain (convper/) launches as it is.  (No error is read: the caller reads hipGetLastError behind
// its last launch.)
void launch_convlarge_grads_update(const LearnArgs& a, hipStream_t s);
int launch_convlarge_sample(const void* counters, uint64_t seed, int batch, int64_t size, int64_t* out, hipStream_t s);

}  // namespace cg
}  // namespace drl
#endif
