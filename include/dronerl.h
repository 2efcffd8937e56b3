/*
 * dronerl.h — C ABI of the MI355X-native batched DroneRL environment
 * (libdronerl.so, hand-written HIP kernels for gfx950).
 *
 * The reference (nyx-ai/droneRL) is pure Python and has no FFI; this ABI is
 * what a Python (ctypes) or any other FFI binds to replace its env hot path:
 *
 *   reference                                            this ABI
 *   torch_impl/env/env.py:68-101   DeliveryDrones.reset   drl_reset
 *   torch_impl/env/env.py:112-215  DeliveryDrones.step    drl_step
 *   torch_impl/env/wrappers.py:55-73 WindowedGridView     drl_obs (or drl_step's fused obs)
 *   torch_impl/env/wrappers.py:34-43 GridView             drl_grid_obs
 *   jax_impl/env/env.py:89-135     DeliveryDrones.reset   drl_reset (batched over envs)
 *   jax_impl/env/env.py:137-250    DeliveryDrones.step    drl_step  (batched over envs)
 *   jax_impl/env/env.py:274-309    DeliveryDrones.get_obs drl_obs
 *   jax_impl/env/env.py:11-35      DroneEnvParams/State   drl_params / drl_state + drl_decode
 *   torch_impl/helpers/rl_helpers.py:12-18 set_seed       drl_reset(reseed=1)
 *   jax_impl/agents/dqn.py:132-146 DQNAgent.act          drl_qnet_act* (drl_qnet_act_eps: epsilon on device)
 *   jax_impl/agents/dqn.py:147-200 train_step / update_target / update_epsilon,
 *   jax_impl/buffers.py:79-93      sample / can_sample,
 *   train_jax.py:68-98             the scan body's learner block   drl_dqn_train
 *   jax_impl/buffers.py:57-77      ReplayBuffer.add_many  drl_replay_add
 *   train_jax.py:55-62             env.step + add_many    drl_step_code_replay (one launch)
 *   train_jax.py:42-62             + the random drones    drl_step_code_replay_synth (drawn in the step)
 *
 * Two layers: stateless calls on caller-owned buffers (drl_reset, drl_step,
 * ...) and library-owned env handles (drl_env_*) that
 * forward to them.
 *
 * Semantics are torch_impl's, bit-exact (state, dict order, done flags, RNG
 * stream), with each env carrying its own CPython-compatible MT19937 stream:
 * env e behaves exactly like `random.seed(seed_base + e); env.reset()` followed
 * by env.step(...) calls in the reference.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers on the current HIP device.
 *  - The caller owns every buffer (state included: size them with
 *    drl_layout_query).  No call allocates, frees or synchronises, so every
 *    call is hipGraph-capturable; all work is enqueued on `stream`.
 *  - Return 0 on success, <0 on error (text: drl_last_error(), thread-local).
 *  - Actions/rewards/dones are indexed by drone index [E][n_drones]; the
 *    state's drone records are kept in dict order (the reference's hidden
 *    iteration order O, env.py:124).
 */
#ifndef DRONERL_H
#define DRONERL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

#define DRL_ABI_VERSION 9
/* Per-env RNG row of `mt` (u32 words, 7104 B):
 *   [0, 624)     MT19937 block 0     the env's CPython stream lives in block
 *   [624, 1248)  MT19937 block 1     mt_index.par; the other block holds the
 *                                    next block (twisted by drl_refill) or scratch
 *   [1248, 1760) respawn-candidate ring (DRL_CAND_SLOTS entries, see drl_refill)
 *   1760         the stream position just after the ring's last entry: MT
 *                index | block << 10 (valid while the ring holds entries)
 *   [1761, 1776) padding (rows 64-B aligned) */
#define DRL_MT_WORDS 1776
#define DRL_MT_BLOCK1 624
#define DRL_MT_RING 1248
#define DRL_MT_RING_END 1760
#define DRL_CAND_SLOTS 512
#define DRL_MAX_DRONES 64
#define DRL_MAX_SIDE 128
#define DRL_MAX_RADIUS 8

/* object codes (common/constants.py:15-19) */
#define DRL_EMPTY 0
#define DRL_SKYSCRAPER 2
#define DRL_STATION 3
#define DRL_DROPZONE 4
#define DRL_PACKET 5

/* error bits written to drl_step's optional err word */
#define DRL_ERR_BAD_ACTION 1   /* action outside [-5, 4] (IndexError in the reference) */
#define DRL_ERR_NO_FREE_CELL 2 /* respawn found no free cell (the reference loops forever) */
#define DRL_ERR_BAD_STATE 4    /* drl_env_set_state: MT index outside [0, 624] (CPython setstate's ValueError;
                                  clamped to 624), or a ground code outside {0, 2, 3, 4, 5} (stored as
                                  its low 4 bits) */
#define DRL_ERR_QNET_RANGE 8   /* drl_qnet_act (DRL_QNET_F32): an input or hidden activation at or beyond fp16's
                                  range (|v| >= 65520) or NaN; that env's Q values are not valid */

/* Env parameters: torch_impl DEFAULT_CONFIG (env.py:28-42) / jax DroneEnvParams
 * (jax env.py:11-26).  `side` is explicit; torch_impl derives it as
 * ceil(sqrt(n_drones / drone_density)) (env.py:75): see drl_side_from_density. */
typedef struct drl_params {
    int32_t side;
    int32_t n_drones;
    int32_t charge;     /* >= 0 */
    int32_t discharge;  /* >= 0 */
    int32_t packets_factor;
    int32_t dropzones_factor;
    int32_t stations_factor;
    int32_t skyscrapers_factor;
    int32_t window_radius; /* 1..DRL_MAX_RADIUS */
    float pickup_reward;
    float delivery_reward;
    float crash_reward;
    float charge_reward;
} drl_params;

/* Buffer geometry for a params set. */
typedef struct drl_layout {
    int32_t side;
    int32_t n_drones;
    int32_t cells;          /* side*side */
    int32_t ground_stride;  /* bytes per env in `ground`: ceil(cells / 2) rounded up to 16 (packed nibbles) */
    int32_t drone_stride;   /* u32 records per env in `drones` (== n_drones) */
    int32_t mt_stride;      /* u32 words per env in `mt` (== DRL_MT_WORDS) */
    int32_t obs_window;     /* 2*radius+1 */
    int32_t obs_floats;     /* floats per observed drone: window^2 * 6 */
    int32_t step_group_lanes; /* wavefront lanes per env in drl_step */
    int32_t step_lds_bytes;   /* dynamic LDS per block (one wavefront) of drl_step */
    int32_t cand_slots;       /* respawn-candidate ring entries per env (DRL_CAND_SLOTS) */
    int32_t refill_every;     /* recommended drl_refill cadence in steps (DRL_STEP_REFILL) */
} drl_layout;

/* Device state of num_envs envs (structure of arrays, env-major).
 *  ground : u8  [E][ground_stride]  object code per cell (row-major k = y*side+x), packed
 *           two cells per byte (ABI 8): cell k in bits 4*(k&1)..+3 of byte k/2
 *           (the codes are < 8; half the HBM bytes of a byte per cell; the
 *           kernels unpack into LDS).  drl_env_get_state / set_state and
 *           BatchedDeliveryDrones.decode / set_state convert to a byte per cell.
 *  drones : u32 [E][n_drones]       one record per drone in dict order:
 *           bits 0-7 y, 8-15 x, 16-23 charge, 24 carrying, 25-31 drone index
 *  mt     : u32 [E][DRL_MT_WORDS]   two MT19937 blocks + the candidate ring (above)
 *  mt_index: u32 [E]                bits 0-9 CPython's MT index (next word; 624 =
 *                                   twist first), bit 10 `par` (the block holding
 *                                   the stream), bits 11-19 ring head, bits 20-29
 *                                   ring count; kept apart so a wave's envs share
 *                                   one cache line.  A plain CPython index (0..624,
 *                                   upper bits 0) is a valid word: block 0, empty ring.
 *
 * The candidate ring is a cache of the env's FUTURE respawn cells: entry k is
 * the k-th (y, x) pair of accepted randint(0, side-1) draws ahead of the
 * stream position (bits 0-13 cell y*side+x, bits 16-25 the MT index after its
 * second draw, bit 26 that index's block).  Those cells depend on the stream
 * alone, not on the board, so drl_refill can draw them in bulk off the step's
 * critical path; drl_step consumes them in order, rejects occupied ones
 * exactly as env.py:226-233 does, and falls back to drawing from the stream
 * itself when the ring runs dry.  Results never depend on the ring's fill
 * level: it only moves MT work out of the step. */
typedef struct drl_state {
    uint8_t* ground;
    uint32_t* drones;
    uint32_t* mt;
    uint32_t* mt_index;
    int64_t num_envs;
} drl_state;

int32_t drl_abi_version(void);
const char* drl_last_error(void);

/* ceil(sqrt(n_drones / drone_density)) in double, as env.py:75 computes it. */
int32_t drl_side_from_density(int32_t n_drones, double drone_density);

/* Validate params and fill the layout.  Errors mirror the reference's
 * ValueErrors (spawn_objects env.py:59-60, sample, jax env.py:96-104). */
int drl_layout_query(const drl_params* p, drl_layout* out);

/* reset() for every env (or every env with d_env_mask[e] != 0).
 * reseed != 0: first re-seed env e's stream as random.seed(seed_base + e)
 * (rl_helpers.py:18), then draw the reset exactly like env.py:68-101.
 * reseed == 0: continue each env's current stream (a plain env.reset()).
 * Ends with a drl_refill of the respawn-candidate rings. */
int drl_reset(const drl_params* p, const drl_state* s, int32_t reseed, uint64_t seed_base,
              const uint8_t* d_env_mask, hipStream_t stream);

/* step(actions) for every env (env.py:112-215).  d_actions int32 [E][n_drones]
 * by drone index; d_rewards f32 [E][n_drones]; d_dones u8 [E][n_drones].
 * d_obs (nullable): fused WindowedGridView observation of drone indices
 * 0..obs_k-1 after the step, f32 [E][obs_k][W][W][6].
 * d_err (nullable): OR-ed DRL_ERR_* bits. */
int drl_step(const drl_params* p, const drl_state* s, const int32_t* d_actions, float* d_rewards,
             uint8_t* d_dones, float* d_obs, int32_t obs_k, int32_t* d_err, hipStream_t stream);

/* drl_step with flags (drl_step == drl_step_ex with flags 0).
 * DRL_STEP_OBS_STREAM: write the observation with streaming (non-temporal)
 * stores, for observations no kernel reads right away (rollout output).
 * Without it the stores are cached, so a consumer launched next (the policy's
 * act) reads them from the caches.  Results are identical either way. */
#define DRL_STEP_OBS_STREAM 1u
/* DRL_STEP_REFILL: launch drl_refill after the step (callers pass it every
 * layout.refill_every steps; the Python env and the env handles do). */
#define DRL_STEP_REFILL 2u
int drl_step_ex(const drl_params* p, const drl_state* s, const int32_t* d_actions, float* d_rewards,
                uint8_t* d_dones, float* d_obs, int32_t obs_k, int32_t* d_err, uint32_t flags,
                hipStream_t stream);

/* num_steps steps (jax_impl run_steps, env/env.py:252-272, with the rewards,
 * dones and observation of every step): identical results to num_steps
 * drl_step calls.  Step t reads d_actions + t * act_step_stride and writes
 * d_rewards / d_dones + t * out_step_stride and d_obs + t * obs_step_stride
 * (element strides; out/obs stride 0 = every step overwrites the same
 * buffer, leaving the last step's).  With layout.step_group_lanes >= 16 the
 * steps run in one launch with the state on chip, written back once at the
 * end (respawns take ring entries while they last, then draw from the
 * stream); narrower groups run one drl_step launch per step with a refill
 * every layout.refill_every steps.  Ends with a drl_refill either way. */
int drl_rollout(const drl_params* p, const drl_state* s, int32_t num_steps, const int32_t* d_actions,
                int64_t act_step_stride, float* d_rewards, uint8_t* d_dones, int64_t out_step_stride, float* d_obs,
                int32_t obs_k, int64_t obs_step_stride, int32_t* d_err, hipStream_t stream);

/* Extend every env's respawn-candidate ring (see drl_state) through the end
 * of the MT block after the stream's: an env whose ring does not reach past
 * the stream's block gets the rest of that block's draws and, twisted into
 * the other block's words, all of the next block's (up to DRL_CAND_SLOTS
 * entries).  Never changes the env's observable state.  drl_reset and
 * drl_mt_set end with one. */
int drl_refill(const drl_params* p, const drl_state* s, hipStream_t stream);

/* The envs' CPython getstate() words: d_words u32 [E][625] = the 624 state
 * words of the stream's block + the MT index (what random.getstate() holds). */
int drl_mt_get(const drl_params* p, const drl_state* s, uint32_t* d_words, hipStream_t stream);
/* random.setstate() for every env from d_words u32 [E][625] (then a refill).
 * An index outside [0, 624] is clamped to 624 and raises DRL_ERR_BAD_STATE in
 * d_err (nullable). */
int drl_mt_set(const drl_params* p, const drl_state* s, const uint32_t* d_words, int32_t* d_err, hipStream_t stream);

/* WindowedGridView observation (wrappers.py:10-31,55-73) of drone indices
 * 0..k-1: f32 [E][k][W][W][6]. */
int drl_obs(const drl_params* p, const drl_state* s, int32_t k, float* d_obs, hipStream_t stream);

/* Policy code (ABI 7): drone index 0's window as one u16 per cell -- object
 * code (bits 0-2, walls as DRL_SKYSCRAPER) | ((charge+1) | carry << 7) << 3
 * (0 above: no drone) -- in four groups of ceil(W*W/4) cells, each padded
 * with zero codes to a multiple of 8.  Bytes per env (16-B multiple): */
int32_t drl_policy_code_bytes(int32_t window_radius);
/* drl_step_ex that also writes the policy code of the state after the step
 * (d_code, 16-B aligned, [E][drl_policy_code_bytes]): what drl_qnet_act_code
 * reads instead of the observation.  With d_obs non-NULL the observation
 * (obs_k >= 1) is written as well; with d_obs NULL the code alone (obs_k
 * ignored): a consumer that only needs drone 0's window skips the f32 rows
 * (6 floats per cell) entirely.  d_code NULL: exactly drl_step_ex. */
int drl_step_code(const drl_params* p, const drl_state* s, const int32_t* d_actions, float* d_rewards,
                  uint8_t* d_dones, float* d_obs, int32_t obs_k, void* d_code, int32_t* d_err, uint32_t flags,
                  hipStream_t stream);
/* Policy code rows -> drone index 0's observation, f32 [n][W][W][6] exactly
 * as drl_obs writes it (a replay buffer of codes decodes its samples). */
int drl_code_decode(int32_t window_radius, const void* d_code, int64_t n, float* d_obs, hipStream_t stream);
/* Measurement helper (the measured copy-kernel peak beside
 * the spec): mode 0 copies `bytes` from d_src to d_dst, mode 1 only reads
 * d_src (d_dst, at least `bytes` long, may be written).  A plain float4
 * copy: one 16-B element per lane, a grid over the buffer.  Time it with
 * events on `stream`. */
int drl_hbm_probe(const void* d_src, void* d_dst, int64_t bytes, int32_t mode, hipStream_t stream);
/* drl_obs that also writes the policy code (d_code nullable); d_obs NULL:
 * the code alone (k ignored). */
int drl_obs_code(const drl_params* p, const drl_state* s, int32_t k, float* d_obs, void* d_code, hipStream_t stream);

/* Multi-agent evaluation (drone_evaluator.py:97-204; dronerl_amd/evaluator.py): every drone driven by its own
 * policy.
 * drl_obs_code_all: the policy code of EVERY drone index of every env, d_codes u8
 * [n_drones][E][drl_policy_code_bytes(window_radius)], drone-major, 16-B aligned.  Row (d, e) is bit for bit
 * the row drl_obs_code writes for an env in which drone index d stands where index 0 does: the same u16 cell
 * encoding, groups and zero padding, walls as DRL_SKYSCRAPER, centred on drone INDEX d (not dict slot d).
 * Drone d's block is a contiguous run of code rows, so drl_qnet_act_code / drl_convnet_act / drl_widenet_act
 * read it unchanged (d_actions + d, action_stride = n_drones).  Reads s->ground and s->drones only; num_envs
 * must be >= 1. */
int drl_obs_code_all(const drl_params* p, const drl_state* s, void* d_codes, hipStream_t stream);
/* One step's rewards into running scores, in the reference's arithmetic (a float64 array += Python doubles):
 * d_scores f64 [E][n_drones] += v, where v is the first of crash, charge, pickup, delivery whose f32 rounding
 * equals the f32 reward d_rewards[e][d] (drl_step's output), else 0 for a zero reward, else the f32 widened.
 * One f64 add per element per call, so a sequence of calls equals numpy's `scores += step_rewards` bit for
 * bit. */
int drl_score_add(const float* d_rewards, int64_t num_envs, int32_t n_drones, double crash_reward, double charge_reward,
                  double pickup_reward, double delivery_reward, double* d_scores, hipStream_t stream);

/* GridView observation (wrappers.py:10-31,34-43): the [side][side][6] f32
 * base grid of every env (each drone of an env sees the same grid):
 * d_grid f32 [E][side][side][6], channels as drl_obs, no wall padding. */
int drl_grid_obs(const drl_params* p, const drl_state* s, float* d_grid, hipStream_t stream);

/* Decode drone records to per-index vectors (jax DroneEnvState fields):
 * d_order[E][N] = drone index at dict position; y/x/charge/carry [E][N] by
 * drone index.  Any output may be NULL. */
int drl_decode(const drl_params* p, const drl_state* s, int32_t* d_order, int32_t* d_y, int32_t* d_x,
               int32_t* d_charge, uint8_t* d_carry, hipStream_t stream);

/* Inverse of drl_decode (hand-built states, as jax_tests/test_env.py:14-110 do).
 * charge must lie in [0, 100]. */
int drl_encode(const drl_params* p, const drl_state* s, const int32_t* d_order, const int32_t* d_y,
               const int32_t* d_x, const int32_t* d_charge, const uint8_t* d_carry, hipStream_t stream);

/* Synthetic uniform actions in {0..4} from a counter hash of
 * (seed, step, env_offset + e, drone) — identical to the oracle's stream. */
int drl_synth_actions(uint64_t seed, uint64_t step, int64_t env_offset, int64_t num_envs, int32_t n_drones,
                      int32_t* d_actions, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Env handles: the library owns the state of num_envs
 * envs on one device; the caller owns actions/rewards/dones/obs.  Every call
 * except create/destroy/errors is asynchronous on `stream` and allocation-free.
 * A handle is single-threaded; use one per device/process.
 *
 *   B2 row                      here
 *   drl_create/drl_destroy      drl_env_create / drl_env_destroy
 *   drl_reset(env, mask)        drl_env_reset (set_seed: drl_env_seed)
 *   drl_step(env, ...)          drl_env_step / drl_env_step_obs (fused obs)
 *   drl_obs(env, k, obs)        drl_env_obs
 *   drl_get_state/set_state     drl_env_get_state / drl_env_set_state
 * ------------------------------------------------------------------------ */
typedef struct drl_env drl_env;

/* SoA view of an env batch (device pointers, dense, env-major):
 *  ground u8 [E][side*side]; order/y/x/charge i32 [E][n_drones] (order = drone
 *  index at dict position, the rest by drone index); carry u8 [E][n_drones];
 *  mt u32 [E][625] = CPython's getstate() words 0..623 + index. */
typedef struct drl_state_view {
    uint8_t* ground;
    int32_t* order;
    int32_t* y;
    int32_t* x;
    int32_t* charge;
    uint8_t* carry;
    uint32_t* mt;
} drl_state_view;

/* Allocate the state of num_envs envs on `device`.  Global env index of env e
 * is env_offset + e (train_jax.py:196-212 sharding); the first drl_env_reset
 * seeds env e as random.seed(base_seed + env_offset + e). */
int drl_env_create(const drl_params* p, int32_t device, int64_t num_envs, int64_t env_offset, uint64_t base_seed,
                   drl_env** out);
int drl_env_destroy(drl_env* env);
/* set_seed (rl_helpers.py:12-18): the next reset re-seeds from base_seed. */
int drl_env_seed(drl_env* env, uint64_t base_seed);
/* reset() (env.py:68-101) of every env, or of envs with d_env_mask[e] != 0
 * (the first reset after create/seed must cover every env). */
int drl_env_reset(drl_env* env, const uint8_t* d_env_mask, hipStream_t stream);
/* step() (env.py:112-215): actions i32, rewards f32, dones u8, [E][n_drones]. */
int drl_env_step(drl_env* env, const int32_t* d_actions, float* d_rewards, uint8_t* d_dones, hipStream_t stream);
/* step() + the WindowedGridView observation of drone indices 0..k-1 after it
 * (cached stores at layout.step_group_lanes 8 or less, streaming stores at 16
 * and more: the faster mode when the policy reads the observation next). */
int drl_env_step_obs(drl_env* env, const int32_t* d_actions, float* d_rewards, uint8_t* d_dones, int32_t k,
                     float* d_obs, hipStream_t stream);
/* WindowedGridView observation (wrappers.py:55-73): f32 [E][k][W][W][6]. */
int drl_env_obs(drl_env* env, int32_t k, float* d_obs, hipStream_t stream);
/* GridView observation (wrappers.py:34-43): f32 [E][side][side][6]. */
int drl_env_grid_obs(drl_env* env, float* d_grid, hipStream_t stream);
/* Copy the state out to / in from a caller-owned SoA view (NULL fields are
 * skipped by get_state; set_state needs all of them and trusts their
 * validity: positions on the grid, distinct cells, charge in [0, 100]; ground
 * codes are common/constants.py Object values {0, 2, 3, 4, 5} (< 8: the
 * packed ground holds a nibble per cell, the policy code 3 bits); an MT index
 * outside [0, 624] is clamped to 624, and a ground code outside that set is
 * stored as its low 4 bits; both raise DRL_ERR_BAD_STATE in the handle's
 * error word). */
int drl_env_get_state(drl_env* env, const drl_state_view* v, hipStream_t stream);
int drl_env_set_state(drl_env* env, const drl_state_view* v, hipStream_t stream);
/* The handle's raw buffers, params and layout (any output may be NULL). */
int drl_env_state(const drl_env* env, drl_state* s, drl_params* p, drl_layout* L);
/* Synchronise `stream`, read the OR of DRL_ERR_* bits raised by steps, and
 * clear them when `clear` != 0. */
int drl_env_errors(drl_env* env, int32_t* flags, int32_t clear, hipStream_t stream);

/* ------------------------------------------------------------------------
 * DQN consumer of the observation, on MFMA: the dense Q-network of jax_impl/agents/dqn.py:47-63
 * (Dense(h) + ReLU per hidden layer, then Dense(n_actions)) and the
 * epsilon-greedy act of dqn.py:132-146 for every env (train_jax.py:42-49:
 * drone 0 follows the agent), plus ReplayBuffer.add_many (buffers.py:57-80).
 *
 * Precision (drl_qnet_desc.precision):
 *   DRL_QNET_BF16: bf16 operands, f32 accumulation (one MFMA per tile and
 *     K-slice); Q within ~1e-2 relative of the f32 forward.
 *   DRL_QNET_F32: the reference's f32 nets (jax dqn.py:47-63 / torch
 *     dqn.py:44-82 run in f32): every operand v is split exactly enough into
 *     fp16 hi = fp16(v) and lo = fp16((v - hi) * 2^11); products hi*hi go to
 *     one f32 accumulator and hi*lo + lo*hi to a second, combined as
 *     acc_hi + 2^-11 * acc_lo (the lo*lo term, <= 2^-22 relative, is
 *     dropped).  Q matches an f32 forward to f32 rounding (~1e-6 relative).
 *     Range: |weights|, |inputs| and |hidden activations| < 65504 (fp16).
 * ------------------------------------------------------------------------ */
#define DRL_QNET_BF16 0
#define DRL_QNET_F32 1
/* input: DRL_QNET_INPUT_OBS, the f32 observation rows (drl_qnet_act); or
 * DRL_QNET_INPUT_CODE, drone index 0's policy code written by drl_step_code /
 * drl_obs_code (drl_qnet_act_code; DRL_QNET_F32, window radius 2..4).  The
 * weights are the same; the packed layout differs. */
#define DRL_QNET_INPUT_OBS 0
#define DRL_QNET_INPUT_CODE 1
typedef struct drl_qnet_desc {
    int32_t in_features;  /* observation floats, W*W*6 (even, <= 512) */
    int32_t n_hidden;     /* 1..3 hidden layers */
    int32_t hidden[3];    /* widths: multiples of 8 in [8, 128] (the packed image pads each to the next
                           * multiple of 32 with zero rows, columns and biases) */
    int32_t n_actions;    /* 1..8 (Action.num_actions() = 5) */
    int32_t precision;    /* DRL_QNET_BF16 or DRL_QNET_F32 */
    int32_t input;        /* DRL_QNET_INPUT_OBS or DRL_QNET_INPUT_CODE (ABI 7) */
} drl_qnet_desc;

/* Bytes of the packed network (weight fragments + f32 biases; DRL_QNET_F32
 * packs fp16 hi and lo fragments: layer 0's hi and lo sets first when both
 * fit the 160 KB LDS together, else the hi fragments where bf16 ones go and
 * the lo fragments after them).  The layout is opaque to callers. */
int drl_qnet_packed_bytes(const drl_qnet_desc* d, int64_t* bytes);
/* Pack the network once per weight update.  d_weights / d_biases: host arrays
 * of n_hidden + 1 device pointers; layer l weights f32 [out][in] row-major
 * (torch nn.Linear; a flax Dense kernel is its transpose), biases f32 [out].
 * d_packed: 16-byte aligned device buffer of drl_qnet_packed_bytes. */
int drl_qnet_pack(const drl_qnet_desc* d, const float* const* d_weights, const float* const* d_biases, void* d_packed,
                  hipStream_t stream);
/* actions[e * action_stride] = u_e < epsilon ? random action : argmax_a Q(obs_e)
 * for e < num_envs (first maximum on ties, like jnp.argmax).  obs f32 rows of
 * obs_stride floats (8-byte aligned).  u_e and the random action come from a
 * counter hash of (seed, step, env_offset + e).  d_q (nullable): Q f32
 * [num_envs][n_actions].  d_err (nullable): OR-ed DRL_ERR_QNET_RANGE. */
int drl_qnet_act(const drl_qnet_desc* d, const void* d_packed, const float* d_obs, int64_t num_envs,
                 int64_t obs_stride, float epsilon, uint64_t seed, uint64_t step, int64_t env_offset,
                 int32_t* d_actions, int64_t action_stride, float* d_q, int32_t* d_err, hipStream_t stream);
/* drl_qnet_act for column 0 of d_actions [num_envs][n_drones] (contiguous
 * rows), fused with drl_synth_actions(synth_seed, synth_step, env_offset,
 * num_envs, n_drones) for columns 1..n_drones-1: one launch for the
 * train_jax.py:42-49 action row (drone 0 from the agent, the others from the
 * synthetic stream), identical to the two calls in sequence.  n_drones >= 1. */
int drl_qnet_act_synth(const drl_qnet_desc* d, const void* d_packed, const float* d_obs, int64_t num_envs,
                       int64_t obs_stride, float epsilon, uint64_t seed, uint64_t step, int64_t env_offset,
                       int32_t* d_actions, int32_t n_drones, uint64_t synth_seed, uint64_t synth_step, float* d_q,
                       int32_t* d_err, hipStream_t stream);

/* drl_qnet_act for a DRL_QNET_INPUT_CODE net, reading drone index 0's policy
 * code (d_code, drl_policy_code_bytes(radius) per env, as drl_step_code /
 * drl_obs_code write it) instead of the f32 observation: the 0/1 and
 * charge/100 inputs are computed from the code exactly as the observation
 * holds them, so Q is the f32 net's on the same window (to f32 rounding).
 * synth_n > 1: as drl_qnet_act_synth (columns 1..synth_n-1 of d_actions from
 * drl_synth_actions(synth_seed, synth_step), action_stride = synth_n). */
int drl_qnet_act_code(const drl_qnet_desc* d, const void* d_packed, const void* d_code, int64_t num_envs,
                      float epsilon, uint64_t seed, uint64_t step, int64_t env_offset, int32_t* d_actions,
                      int64_t action_stride, int32_t synth_n, uint64_t synth_seed, uint64_t synth_step, float* d_q,
                      int32_t* d_err, hipStream_t stream);

/* Replay ring buffer storage (device, caller-owned): obs/next_obs f32
 * [capacity][obs_floats], actions i32, rewards f32, dones u8 [capacity].
 * Rows are copied bit for bit: policy-code rows (drl_policy_code_bytes / 4
 * words each) store the same way. */
typedef struct drl_replay {
    int64_t capacity;
    int32_t obs_floats;
    float* obs;
    float* next_obs;
    int32_t* actions;
    float* rewards;
    uint8_t* dones;
} drl_replay;

/* add_many: transition i -> slot (cursor + i) % capacity, i < n; strides in
 * elements (e.g. action_stride = n_drones to take drone 0 of [E][n_drones]).
 * With n > capacity only the last `capacity` transitions are written (what a
 * sequential add() loop leaves).  The caller advances cursor by n. */
int drl_replay_add(const drl_replay* r, int64_t cursor, int64_t n, const float* d_obs, int64_t obs_stride,
                   const float* d_next_obs, int64_t next_obs_stride, const int32_t* d_actions, int64_t action_stride,
                   const float* d_rewards, int64_t reward_stride, const uint8_t* d_dones, int64_t done_stride,
                   hipStream_t stream);
/* drl_step_code (no f32 observation) fused with the drl_replay_add of the
 * step's drone-0 transitions, code rows (replaces train_jax.py:55-62's
 * env.step + buffer.add_many pair, jax_impl/buffers.py:57-80): env e lands
 * in slot (cursor + e) % capacity with obs = d_code_prev row e (the rows the
 * act read; another buffer than d_code), next_obs = the code this step
 * writes to d_code, action = d_actions[e * n_drones], reward / done = drone
 * index 0's.  The ring's contents equal drl_step_code + drl_replay_add(obs =
 * d_code_prev, next_obs = d_code, action/reward/done column 0) bit for bit;
 * r->obs_floats * 4 = drl_policy_code_bytes(window_radius), rows 16-byte
 * aligned.  The caller advances cursor by num_envs. */
int drl_step_code_replay(const drl_params* p, const drl_state* s, const int32_t* d_actions, float* d_rewards,
                         uint8_t* d_dones, void* d_code, const void* d_code_prev, const drl_replay* r, int64_t cursor,
                         int32_t* d_err, uint32_t flags, hipStream_t stream);
/* drl_step_code_replay whose drone indices 1..n_drones-1 act as drl_synth_actions(synth_seed, synth_step,
 * env_offset) writes them (train_jax.py:42-49: every drone but drone 0 acts at random; the same counter hash,
 * drawn inside the step): d_actions is read at column 0 only (d_actions[e * n_drones], the agent's action), its
 * other columns are neither read nor written.  Bit for bit drl_synth_actions into d_actions' columns >= 1 +
 * drl_step_code_replay.  In the train loop it replaces drl_qnet_act_synth's columns (no 4 B per drone written
 * by the act and read back by the step). */
int drl_step_code_replay_synth(const drl_params* p, const drl_state* s, const int32_t* d_actions, float* d_rewards,
                               uint8_t* d_dones, void* d_code, const void* d_code_prev, const drl_replay* r,
                               int64_t cursor, uint64_t synth_seed, uint64_t synth_step, int64_t env_offset,
                               int32_t* d_err, uint32_t flags, hipStream_t stream);


/* drl_qnet_act / drl_qnet_act_code with epsilon read from device memory
 * (d_epsilon: e.g. the learner's drl_dqn_counters.epsilon, which drl_dqn_train
 * decays on the device), so a captured graph of the train loop acts with the
 * current schedule.  d_input: the f32 observation rows (obs_stride floats) of
 * a DRL_QNET_INPUT_OBS net, or the policy code of a DRL_QNET_INPUT_CODE net
 * (obs_stride ignored).  synth_n > 1: drl_qnet_act_synth's columns. */
int drl_qnet_act_eps(const drl_qnet_desc* d, const void* d_packed, const void* d_input, int64_t num_envs,
                     int64_t obs_stride, const float* d_epsilon, uint64_t seed, uint64_t step, int64_t env_offset,
                     int32_t* d_actions, int64_t action_stride, int32_t synth_n, uint64_t synth_seed,
                     uint64_t synth_step, float* d_q, int32_t* d_err, hipStream_t stream);

/* ------------------------------------------------------------------------
 * DQN learner (the train half): one drl_dqn_train call is the
 * learner block of one train_jax.py scan step (:68-98):
 *   if current_size >= batch (buffers.py:92-93 can_sample):
 *       batch = sample(replay) (buffers.py:79-90: uniform rows in [0, size));
 *       train_step (jax_impl/agents/dqn.py:147-183): q = Q(obs)[action],
 *       td = reward + gamma * max_a Q_target(next_obs) * (1 - done),
 *       loss = mean((q - td)^2), gradient, optax.adam(learning_rate, beta1,
 *       beta2, adam_eps) update;
 *   if step % target_update_interval == 0: target = tau * online + (1 - tau)
 *       * target (dqn.py:185-190, optax.incremental_update);
 *   if step % epsilon_decay_every == 0: epsilon = max(epsilon * decay, end)
 *       (dqn.py:192-200);
 *   step += 1.
 * The step counter, Adam count, epsilon and bias-correction powers live in the
 * agent block on the device (drl_dqn_counters), so the call is graph-capturable
 * and a replayed graph continues the schedule.  The online net's packed image
 * (drl_qnet_pack's layout, d_packed) is refreshed by the same call, ready for
 * the next act.  Row sampling: a counter hash of (sample_seed, step, row) --
 * the reference's jax.random stream is jax-only.  Numerics: f32 throughout,
 * each product and sum rounded in a fixed order (oracle/dqn_learner.py).
 * Dense nets of drl_qnet_desc (1-3 hidden layers, <= 128 wide, <= 8 actions).
 * ------------------------------------------------------------------------ */
typedef struct drl_dqn_hparams {
    int32_t batch;                  /* sample batch (train_jax.py --batch_size, 8): 1..64 for drl_dqn_train and
                                       drl_convnet_dqn_train, 1..DRL_DQN_LARGE_MAX_BATCH (4096) for
                                       drl_dqn_large_train and drl_convnet_dqn_large_train */
    int32_t target_update_interval; /* >= 1 (--target_update_interval, 10) */
    int32_t epsilon_decay_every;    /* >= 1 (--epsilon_decay_every, 5) */
    int32_t reserved;               /* 0 */
    double gamma;                   /* 0.9 (--gamma) */
    double learning_rate;           /* 1e-3 (--learning_rate) */
    double beta1, beta2, adam_eps;  /* optax.adam defaults 0.9, 0.999, 1e-8 */
    double tau;                     /* 1.0 (--tau) */
    double epsilon_decay, epsilon_end;  /* train_jax.py:133-136; --epsilon_end 0.01 */
    uint64_t sample_seed;
} drl_dqn_hparams;

/* Device counters at counters_off of the agent block. */
typedef struct drl_dqn_counters {
    int32_t step;        /* the scan step (train_jax.py carry `step`) */
    int32_t count;       /* Adam steps taken (optax ScaleByAdamState.count) */
    float epsilon;       /* the act's exploration rate */
    float loss;          /* the last train_step's loss (0 without a sample) */
    double beta1_pow, beta2_pow;  /* beta^count */
    int32_t internal[8]; /* the learner's own: arrival ticket, the step's plan */
} drl_dqn_counters;

/* The agent block (device, caller-owned, one allocation of `bytes`, 16-B
 * aligned): four parameter sets (online, target, Adam mu, Adam nu) of n_params
 * floats each -- layer l's weight [out][in] row-major (torch nn.Linear) at
 * weight_off[l], its bias at bias_off[l] (floats from the set's start) --, the
 * counters, and the learner's scratch. */
typedef struct drl_dqn_layout {
    int64_t n_params;
    int64_t weight_off[4], bias_off[4];
    int64_t online_off, target_off, m_off, v_off;  /* bytes */
    int64_t counters_off, scratch_off, bytes;       /* bytes */
    int32_t grad_workgroups, grad_lds_bytes;        /* the learner launch: workgroups, dynamic LDS (informative) */
} drl_dqn_layout;

int drl_dqn_layout_query(const drl_qnet_desc* d, int32_t batch, drl_dqn_layout* layout);
/* Zero the Adam moments, the counters (a timeout flag included) and the whole
 * scratch (the hand-off granules must start untagged, whether the block comes
 * from hipMalloc or has trained before), epsilon = epsilon_start (dqn.py:116-130:
 * optax.adam's init, epsilon_start).  The caller writes the online and target
 * parameters (the reference initialises them from different keys,
 * dqn.py:114-121).  Synchronises `stream` (a host table is uploaded). */
int drl_dqn_init(const drl_qnet_desc* d, int32_t batch, void* d_agent, float epsilon_start, hipStream_t stream);
/* One learner step on replay `r` holding `size` transitions (current_size,
 * 0 <= size <= capacity).  The replay's rows: f32 observations (obs_floats >=
 * in_features) for a DRL_QNET_INPUT_OBS net, policy code rows
 * (drl_policy_code_bytes / 4 words) for a DRL_QNET_INPUT_CODE one.  d_packed:
 * the online net's packed image (drl_qnet_pack of the online set).
 * The launch's grad_workgroups poll each other's hand-offs, so they must be
 * co-resident: the call fails (-1) on a device that cannot hold them all at
 * once (e.g. a 32-CU partition).  A workgroup that gives up on a hand-off
 * (a bounded wait) sets internal[5] of the counters; from then on every call
 * returns on the device without touching the block, until drl_dqn_init. */
int drl_dqn_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                  const struct drl_replay* r, int64_t size, hipStream_t stream);
/* A drl_replay_add batch (its arguments; strides in elements, obs strides in
 * 32-bit words). */
typedef struct drl_replay_batch {
    int64_t cursor, n;
    const void* obs;
    int64_t obs_stride;
    const void* next_obs;
    int64_t next_obs_stride;
    const int32_t* actions;
    int64_t action_stride;
    const float* rewards;
    int64_t reward_stride;
    const uint8_t* dones;
    int64_t done_stride;
} drl_replay_batch;
/* drl_dqn_train as if drl_replay_add(r, fresh->cursor, fresh->n, ...) had
 * already run (`size` counts its rows): the rows that add writes are read
 * from its own buffers, so the add may run concurrently on another stream
 * (the learner reads no slot it writes). */
int drl_dqn_train_fresh(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                        const struct drl_replay* r, int64_t size, const drl_replay_batch* fresh, hipStream_t stream);

/* The `batch` replay slots (int64, [0, size)) the next drl_dqn_train on this
 * block draws: the same counter hash of (sample_seed, step, row), with the step
 * the counters hold when this launch runs on `stream`.  A sharded caller
 * gathers those rows from the ranks that own them before the train call
 * (the global learner; jax_impl/buffers.py:79-90 sample over
 * one global ring, train_jax.py:196-212). */
int drl_dqn_sample_rows(const drl_qnet_desc* d, const drl_dqn_hparams* h, const void* d_agent, int64_t size,
                        int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * The same learner for replay batches up to DRL_DQN_LARGE_MAX_BATCH: one
 * drl_dqn_large_train call is the learner block written above drl_dqn_train,
 * with its semantics and its arithmetic bit for bit (the rows of a step are
 * the same counter hash's, so at batch <= 64 both calls leave the same
 * parameter sets, counters and packed image).  Where drl_dqn_train is one
 * launch whose workgroups hand a batch of <= 64 rows to each other through
 * LDS, this is a fixed chain of stream-ordered launches on `stream` (the rows,
 * each layer's forward of both nets, the TD error, each layer's backward, the
 * parameter update, the counters, the re-pack): no workgroup waits for
 * another, nothing needs to be co-resident, no float atomic is used, nothing
 * is allocated and nothing synchronises, so the call is graph-capturable and
 * a replayed graph continues the schedule.  With size < batch only the target
 * blend (when due) and the counters run.  The same drl_dqn_hparams,
 * drl_dqn_counters, drl_replay and row kinds (f32 rows for a
 * DRL_QNET_INPUT_OBS net, policy-code rows for a DRL_QNET_INPUT_CODE one);
 * dense nets of drl_qnet_desc.  Every argument is validated before any device
 * work.
 * ------------------------------------------------------------------------ */
#define DRL_DQN_LARGE_MAX_BATCH 4096
/* Host only.  drl_dqn_layout with drl_dqn_layout_query's parameter-set offsets
 * (n_params, weight_off, bias_off, online_off .. counters_off) and a scratch
 * sized for `batch` (the rows' decoded inputs, both nets' activations, the
 * deltas); grad_workgroups = grad_lds_bytes = 0. */
int drl_dqn_large_layout_query(const drl_qnet_desc* d, int32_t batch, drl_dqn_layout* layout);
/* drl_dqn_init for this agent block: the Adam moments and the counters from
 * zero, epsilon = epsilon_start; the caller writes the online and target
 * parameters.  Stream-ordered: it does not synchronise. */
int drl_dqn_large_init(const drl_qnet_desc* d, int32_t batch, void* d_agent, float epsilon_start, hipStream_t stream);
/* One learner step (drl_dqn_train's arguments).  After the call d_packed is
 * byte for byte drl_qnet_pack of the online set. */
int drl_dqn_large_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                        const struct drl_replay* r, int64_t size, hipStream_t stream);
/* drl_dqn_sample_rows for this agent block: h->batch slots. */
int drl_dqn_large_sample_rows(const drl_qnet_desc* d, const drl_dqn_hparams* h, const void* d_agent, int64_t size,
                              int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Prioritized experience replay (Schaul et al. 2016, proportional variant)
 * for drl_dqn_large_train's learner: the reference samples uniformly
 * (jax_impl/buffers.py:79-90); this is an option beside it.  A priority sum
 * tree over the ring's slots lives in one caller-owned device block
 * (drl_per_layout, 16-B aligned):
 *   P = the smallest power of two >= capacity; float tree[2P] in heap order:
 *   tree[1] the root, node i's children 2i and 2i + 1, slot s's leaf
 *   tree[P + s], tree[0] unused.  A leaf holds the slot's priority already
 *   raised to alpha (0.0: never written, or a pad leaf s >= capacity); every
 *   internal node is tree[2i] + tree[2i + 1] as one f32 addition.
 * pmax (f32, 1.0 after drl_per_init) is the largest priority ever assigned;
 * new transitions enter with it (drl_per_mark_new after any add).  The block
 * also holds one step's drawn slots (int64 [batch]), their importance weights
 * (f32 [batch], already divided by wmax), wmax, and the rows' |TD error|.
 * Every call validates its arguments before any device work, is
 * stream-ordered, allocates nothing and does not synchronise.
 * ------------------------------------------------------------------------ */
#define DRL_PER_MAX_CAPACITY (1 << 24)
typedef struct drl_per_hparams {
    double alpha;        /* >= 0: priority = (|td error| + eps)^alpha; 0 = uniform over the written slots */
    double beta0;        /* in [0, 1]: the importance exponent at step 0 */
    int64_t beta_steps;  /* >= 0: beta = beta0 + (1 - beta0) * min(1, step / beta_steps); 0: beta0 throughout */
    double eps;          /* >= 0 */
} drl_per_hparams;
typedef struct drl_per_layout {
    int64_t capacity, leaves;  /* leaves = P */
    int32_t batch, reserved;
    int64_t tree_off, pmax_off, wmax_off, slots_off, weights_off, absd_off, bytes;  /* bytes, multiples of 16 */
} drl_per_layout;
/* Host only.  capacity in [1, DRL_PER_MAX_CAPACITY], batch in [1, DRL_DQN_LARGE_MAX_BATCH]. */
int drl_per_layout_query(int64_t capacity, int32_t batch, drl_per_layout* layout);
/* The tree zeroed, pmax = 1. */
int drl_per_init(int64_t capacity, int32_t batch, void* d_per, hipStream_t stream);
/* The leaves of slots [cursor, cursor + count) mod capacity = pmax (drl_replay_add's slots for the same cursor
 * and n; count > capacity marks every slot).  The internal nodes are refreshed by the next rebuild. */
int drl_per_mark_new(int64_t capacity, int32_t batch, void* d_per, int64_t cursor, int64_t count, hipStream_t stream);
/* Every internal node from the leaves (two launches at most). */
int drl_per_rebuild(int64_t capacity, int32_t batch, void* d_per, hipStream_t stream);
/* The block's slots, weights and wmax for the step the counters at d_counters (a drl_dqn_counters on the device:
 * an agent block's counters_off) hold, from a rebuilt tree with a positive root -- stratified, one row per
 * stratum; all f32 unless stated:
 *   h = splitmix64(seed ^ splitmix64(((uint64)(uint32)step << 16) | b))      (drl_dqn_sample_rows' hash)
 *   u = (float)(h >> 40) * 2^-24;  m = ((float)b + u) / (float)batch * tree[1]
 *   i = 1; while i < P: l = tree[2i], r = tree[2i + 1];
 *                       if r == 0 or m < l: i = 2i; else: m = m - l, i = 2i + 1
 *   slot = i - P     (the walk never enters a node of value 0.0, so the slot has been written)
 *   w = (float)pow((double)size * ((double)tree[P + slot] / (double)tree[1]), -beta)   (beta: double)
 *   wmax = max_b w;  weights[b] = w / wmax
 * size in [1, capacity]: the ring's current size. */
int drl_per_sample(int64_t capacity, int32_t batch, void* d_per, const drl_per_hparams* ph, uint64_t seed,
                   const void* d_counters, int64_t size, hipStream_t stream);
/* drl_dqn_large_train on prioritized rows (its arguments, agent block, launch chain and arithmetic; dense nets
 * of drl_qnet_desc, f32 or policy-code rows, batch 1..4096; d_per laid out for (r->capacity, h->batch)):
 * rebuild, sample (seed h->sample_seed, the agent's counters), the rows at the drawn slots, each layer's forward
 * of both nets, the TD error d = q - td with the row's squared error w * (d * d) and the Q head's delta
 * w * ((d + d) / batch), the priority update, each layer's backward, the update, the counters, the re-pack.
 * The priority update: p = (float)pow((double)|d| + eps, alpha), at most 2^64 (a NaN becomes 2^64), stored in the
 * slot's leaf; a slot drawn by several rows takes the largest of their values; pmax = max(pmax, p).  With
 * size < h->batch it is drl_dqn_large_train's no-sample step and the tree is left alone.  alpha = 0 and
 * beta0 = 0, beta_steps = 0 give weights and priorities of exactly 1.0.  Graph-capturable. */
int drl_dqn_per_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph, void* d_agent,
                      void* d_packed, const struct drl_replay* r, int64_t size, void* d_per, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Convolutional Q-networks (torch_impl/agents/dqn.py:85-159 ConvQNetwork,
 * jax_impl/agents/dqn.py:66-94; sample_models/dqn-agent-5 is one): inference
 * (drl_convnet_pack, drl_convnet_act) and, below, the learner
 * (drl_convnet_dqn_*):
 *   x: [E][W][W][6] f32 window (drl_obs's layout, channels last)
 *   per conv layer: y[oy][ox][co] = relu(b[co] + sum_{ky,kx,ci} w[co][ci][ky][kx]
 *       * x[oy*s + ky - p][ox*s + kx - p][ci]), x = 0 outside the map, output
 *       side (side + 2p - k) / s + 1 (floor);
 *   flatten in torch order (co*H*W + oy*W + ox; jax dqn.py:82 transposes to the
 *       same), 0..2 hidden Dense + ReLU, Dense(n_actions).
 * Numerics are DRL_QNET_F32's (fp16 hi/lo split operands, three MFMAs per
 * product tile): Q matches an f32 forward to f32 rounding.
 * Limits (each refused by name when the description is validated, by every
 * call below): window odd in [3, 9]; 1..3 conv layers with out_channels in
 * [1, 32], square kernel_size in [1, 5], stride in [1, 3], padding in [0, 4],
 * every map side >= 1; 0..2 dense widths, multiples of 8 in [8, 128];
 * n_actions in [1, 8]; input DRL_QNET_INPUT_OBS or DRL_QNET_INPUT_CODE (a
 * 5x5, 7x7 or 9x9 window); one env's maps (with their zero halos) within the
 * 160 KB LDS of a CU.
 * ------------------------------------------------------------------------ */
#define DRL_CONVNET_MAX_CONV 3
#define DRL_CONVNET_MAX_DENSE 2
typedef struct drl_convnet_conv {
    int32_t out_channels, kernel_size, stride, padding;
} drl_convnet_conv;
typedef struct drl_convnet_desc {
    int32_t window;   /* W: the observation is [W][W][6] */
    int32_t n_conv;
    drl_convnet_conv conv[DRL_CONVNET_MAX_CONV];
    int32_t n_dense;  /* hidden dense layers after the flatten (0: the flatten feeds the Q head) */
    int32_t dense[DRL_CONVNET_MAX_DENSE];
    int32_t n_actions;
    int32_t input;    /* DRL_QNET_INPUT_OBS or DRL_QNET_INPUT_CODE */
} drl_convnet_desc;

/* Bytes of the packed network (opaque: fp16 hi and lo MFMA fragments of every
 * layer, f32 biases, the conv layers' gather tables, a status word). */
int drl_convnet_packed_bytes(const drl_convnet_desc* d, int64_t* bytes);
/* Pack the parameters (f32, torch layout): d_conv_w[l] [out][in][kh][kw] and
 * d_conv_b[l] [out] for the n_conv conv layers, d_dense_w[l] [out][in] and
 * d_dense_b[l] [out] for the n_dense + 1 dense layers (the Q head last); host
 * arrays of device pointers.  The zero padding of every GEMM and the flatten's
 * permutation (the first dense layer's columns) are folded into the image.  A
 * weight with |w| >= 65504 (or not finite) sets the image's status word, which
 * every act then reports as DRL_ERR_QNET_RANGE.  d_packed: 16-byte aligned. */
int drl_convnet_pack(const drl_convnet_desc* d, const float* const* d_conv_w, const float* const* d_conv_b,
                     const float* const* d_dense_w, const float* const* d_dense_b, void* d_packed, hipStream_t stream);
/* drl_qnet_act's epsilon-greedy rule on the conv net's Q values, one launch
 * for every env: the same counter hash of (seed, step, env_offset + e), the
 * first maximum on ties.  d_input: f32 rows of obs_stride floats (8-byte
 * aligned, obs_stride even and >= W*W*6) for a DRL_QNET_INPUT_OBS net; drone
 * index 0's policy code (drl_policy_code_bytes per env, 16-byte aligned;
 * obs_stride ignored) for a DRL_QNET_INPUT_CODE net, decoded exactly as
 * drl_code_decode does, so Q is bit for bit the obs net's.  d_epsilon
 * (nullable): the exploration rate read on the device instead of `epsilon`.
 * d_q (nullable): f32 [num_envs][n_actions].  d_err (nullable): OR-ed
 * DRL_ERR_QNET_RANGE when a staged input or an activation has |v| >= 65520 or
 * is NaN.  Allocates nothing and does not synchronise. */
int drl_convnet_act(const drl_convnet_desc* d, const void* d_packed, const void* d_input, int64_t num_envs,
                    int64_t obs_stride, float epsilon, const float* d_epsilon, uint64_t seed, uint64_t step,
                    int64_t env_offset, int32_t* d_actions, int64_t action_stride, float* d_q, int32_t* d_err,
                    hipStream_t stream);

/* ------------------------------------------------------------------------
 * DQN learner for conv nets: one drl_convnet_dqn_train call is the learner
 * block of one train_jax.py scan step (:68-98) with network_type == 'conv',
 * with exactly the semantics written above drl_dqn_train (sample when size >=
 * batch, q = Q(obs)[action], td = reward + gamma * max_a Q_target(next_obs) *
 * (1 - done), loss = mean((q - td)^2), its gradient with respect to every conv
 * and dense parameter, optax.adam, the target blend every
 * target_update_interval steps, the epsilon decay every epsilon_decay_every
 * steps, step += 1; with size < batch nothing trains and only the schedule
 * advances).  The same drl_dqn_hparams, drl_dqn_counters, drl_replay and row
 * draw (the counter hash of (sample_seed, step, row)).  relu'(0) = 0.
 * The call is a fixed sequence of stream-ordered launches (rows: one
 * workgroup per sampled row, forward and backward to every layer's deltas;
 * update: one thread per dense parameter and one wave per conv parameter,
 * the gradient summed in a fixed order, Adam, the target blend; counters; the
 * pack kernel on the online set): no workgroup waits for another, no float atomics, so the
 * result is reproducible bit for bit; it allocates nothing, does not
 * synchronise and can be captured into a graph, whose replays continue the
 * schedule.  Numerics: f32, each product and sum rounded on its own.
 * Limits: drl_convnet_desc's, batch in [1, 64], and one row's input,
 * activations and deltas of every layer (4 bytes each, each layer's rounded
 * up to 16 bytes) within DRL_CONVNET_DQN_ROW_BYTES_MAX, the LDS one workgroup
 * of the rows kernel takes; a larger net is refused by name.
 * ------------------------------------------------------------------------ */
#define DRL_CONVNET_DQN_MAX_LAYERS 6 /* DRL_CONVNET_MAX_CONV + DRL_CONVNET_MAX_DENSE + the Q head */
#define DRL_CONVNET_DQN_ROW_BYTES_MAX 65536
/* The agent block (device, caller-owned, one allocation of `bytes`, 16-B
 * aligned): four parameter sets (online, target, Adam mu, Adam nu) of n_params
 * floats each -- layer l's weight at weight_off[l], its bias at bias_off[l]
 * (floats from the set's start); the conv layers first ([out][in][k][k]), then
 * the dense layers ([out][in], the first one's columns in torch's flatten
 * order, the Q head last): torch layouts --, one drl_dqn_counters at
 * counters_off, and the learner's scratch. */
typedef struct drl_convnet_dqn_layout {
    int64_t n_params;
    int32_t n_layers, row_bytes;  /* layers; the per-row working set (informative) */
    int64_t weight_off[DRL_CONVNET_DQN_MAX_LAYERS], bias_off[DRL_CONVNET_DQN_MAX_LAYERS];
    int64_t online_off, target_off, m_off, v_off;  /* bytes */
    int64_t counters_off, scratch_off, bytes;       /* bytes */
} drl_convnet_dqn_layout;

/* Host only (works without a device). */
int drl_convnet_dqn_layout_query(const drl_convnet_desc* d, int32_t batch, drl_convnet_dqn_layout* layout);
/* Zero the Adam moments, the counters and the scratch, epsilon = epsilon_start.
 * The caller writes the online and target parameters.  Does not synchronise. */
int drl_convnet_dqn_init(const drl_convnet_desc* d, int32_t batch, void* d_agent, float epsilon_start,
                         hipStream_t stream);
/* One learner step on replay `r` holding `size` transitions (0 <= size <=
 * capacity).  The replay's rows: f32 observations (obs_floats >= W*W*6) for a
 * DRL_QNET_INPUT_OBS description, policy code rows (drl_policy_code_bytes / 4
 * words) for a DRL_QNET_INPUT_CODE one.  d_packed: the online net's packed
 * image; after the call it is byte for byte drl_convnet_pack of the online
 * set (a weight outside the fp16 split range raises its status word). */
int drl_convnet_dqn_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                          const struct drl_replay* r, int64_t size, hipStream_t stream);
/* drl_dqn_sample_rows for this agent block. */
int drl_convnet_dqn_sample_rows(const drl_convnet_desc* d, const drl_dqn_hparams* h, const void* d_agent,
                                int64_t size, int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * The same learner for replay batches up to DRL_CONVNET_DQN_LARGE_MAX_BATCH:
 * the four calls of drl_convnet_dqn_* with the same arguments, the same
 * drl_convnet_desc, drl_dqn_hparams, drl_dqn_counters, drl_replay, row kinds
 * (f32 or policy code) and row draw, and the same drl_convnet_dqn_layout
 * with a larger scratch.  One call is a fixed chain of stream-ordered kernel
 * launches (rows: one workgroup per sampled row; the dense layers' and the
 * conv layers' partial gradients per chunk of 64 rows; update; counters; the
 * pack kernel): no workgroup waits for another, no float atomics, no memset,
 * nothing allocated, no synchronisation; it can be captured into a graph,
 * whose replays continue the schedule.  With size < batch only the target
 * blend (when due) and the counters run.
 * The reduction order is fixed: a row's forward, TD and backward are
 * drl_convnet_dqn_train's, the head delta (d + d) / float(batch); rows are
 * cut into chunks of 64 (chunk c: rows 64 c .. min(64 c + 63, batch - 1)) and
 * a chunk's partial gradient of a parameter is summed exactly as
 * drl_convnet_dqn_train sums its whole gradient; g = p[0] + p[1] + ... in
 * chunk order, then Adam and the blend; the loss is the chunks' squared-error
 * sums (rows in order) added in chunk order, / float(batch).  At batch <= 64
 * there is one chunk and the call equals drl_convnet_dqn_train bit for bit
 * (the four sets, the counters, the loss, the packed image).
 * Limits, each refused by name before any device work: drl_convnet_desc's,
 * batch in [1, DRL_CONVNET_DQN_LARGE_MAX_BATCH], a row's working set within
 * DRL_CONVNET_DQN_ROW_BYTES_MAX.  The block's scratch holds 16 KB of squared
 * errors, batch x row_bytes of rows and ceil(batch / 64) x n_params x 4 bytes
 * of partial gradients (n_params rounded up to 4): a few hundred MB at the
 * corners (batch 4096 with 64 KB rows: 256 MB of rows).
 * ------------------------------------------------------------------------ */
#define DRL_CONVNET_DQN_LARGE_MAX_BATCH 4096
/* Host only (works without a device). */
int drl_convnet_dqn_large_layout_query(const drl_convnet_desc* d, int32_t batch, drl_convnet_dqn_layout* layout);
/* Zero the Adam moments and the counters, epsilon = epsilon_start.  The caller
 * writes the online and target parameters.  Does not synchronise. */
int drl_convnet_dqn_large_init(const drl_convnet_desc* d, int32_t batch, void* d_agent, float epsilon_start,
                               hipStream_t stream);
/* drl_convnet_dqn_train's arguments and result at batches up to 4096. */
int drl_convnet_dqn_large_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                                const struct drl_replay* r, int64_t size, hipStream_t stream);
/* drl_dqn_sample_rows for this agent block. */
int drl_convnet_dqn_large_sample_rows(const drl_convnet_desc* d, const drl_dqn_hparams* h, const void* d_agent,
                                      int64_t size, int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Wide dense Q-networks: hidden widths up to DRL_WIDENET_MAX_WIDTH
 * (run_jax_sweep.py trains hidden_layers = (256, 128, 64)), beside drl_qnet_*
 * whose act kernels keep layer 0 in LDS and stop at 128.  The same net
 * (in_features -> hidden... (ReLU) -> n_actions, torch layout [out][in]) with
 * DRL_QNET_F32's numerics: every operand v split into fp16 hi = fp16(v) and
 * lo = fp16((v - hi) * 2^11), three MFMAs per product tile, the layer's value
 * (acc + 2^-11 acl) + bias; Q matches an f32 forward to f32 rounding.  The
 * packed image (up to ~1.1 MB) does not fit a CU's LDS: the act reads its
 * weight fragments from global memory (L2), each read serving every env tile
 * of the workgroup.  The description takes narrow nets too.
 * Limits (each refused by name, by every call below): in_features even in
 * [2, 512]; 1..3 hidden widths, multiples of 8 in [8, DRL_WIDENET_MAX_WIDTH];
 * n_actions in [1, 8]; input DRL_QNET_INPUT_OBS, or DRL_QNET_INPUT_CODE with
 * in_features = W*W*6 for W in 5, 7, 9.
 * ------------------------------------------------------------------------ */
#define DRL_WIDENET_MAX_WIDTH 256
typedef struct drl_widenet_desc {
    int32_t in_features;  /* even, 2..512 */
    int32_t n_hidden;     /* 1..3 */
    int32_t hidden[3];    /* multiples of 8 in [8, DRL_WIDENET_MAX_WIDTH] */
    int32_t n_actions;    /* 1..8 */
    int32_t input;        /* DRL_QNET_INPUT_OBS or DRL_QNET_INPUT_CODE (5x5, 7x7, 9x9 window) */
} drl_widenet_desc;

/* Bytes of the packed network (opaque: every layer's fp16 hi and lo MFMA
 * fragments with widths and K padded with zeros, f32 biases, a 16-byte status
 * vector). */
int drl_widenet_packed_bytes(const drl_widenet_desc* d, int64_t* bytes);
/* drl_qnet_pack's arguments: d_weights[l] [out][in] and d_biases[l] [out], f32,
 * host arrays of n_hidden + 1 device pointers.  A weight with |w| >= 65504 (or
 * not finite) sets the image's status word, which every act then reports as
 * DRL_ERR_QNET_RANGE.  d_packed: 16-byte aligned. */
int drl_widenet_pack(const drl_widenet_desc* d, const float* const* d_weights, const float* const* d_biases,
                     void* d_packed, hipStream_t stream);
/* drl_convnet_act's arguments and rule: the epsilon-greedy choice on the net's
 * Q values, one launch for every env, with the other acts' exploration stream
 * (the counter hash of (seed, step, env_offset + e); the first maximum on
 * ties).  d_input: f32 rows of obs_stride floats (8-byte aligned, obs_stride
 * even and >= in_features) for a DRL_QNET_INPUT_OBS net; drone index 0's
 * policy code (drl_policy_code_bytes per env, 16-byte aligned; obs_stride
 * ignored) for a DRL_QNET_INPUT_CODE net, decoded exactly as drl_code_decode
 * does, so Q is bit for bit the obs net's.  d_epsilon (nullable): the
 * exploration rate read on the device instead of `epsilon`.  d_q (nullable):
 * f32 [num_envs][n_actions].  d_err (nullable): OR-ed DRL_ERR_QNET_RANGE when
 * an input or a hidden activation has |v| >= 65520 or is NaN.  Allocates
 * nothing, does not synchronise, no workgroup waits for another. */
int drl_widenet_act(const drl_widenet_desc* d, const void* d_packed, const void* d_input, int64_t num_envs,
                    int64_t obs_stride, float epsilon, const float* d_epsilon, uint64_t seed, uint64_t step,
                    int64_t env_offset, int32_t* d_actions, int64_t action_stride, float* d_q, int32_t* d_err,
                    hipStream_t stream);
/* The learner: drl_dqn_large_*'s launch chain, agent block (drl_dqn_layout),
 * semantics and arithmetic (bit for bit at the widths both take) for a
 * drl_widenet_desc; batch in [1, DRL_DQN_LARGE_MAX_BATCH].  After
 * drl_widenet_dqn_train d_packed is byte for byte drl_widenet_pack of the
 * online set.  Nothing is allocated, nothing synchronises, no workgroup waits
 * for another, no float atomic is used: the calls are graph-capturable. */
int drl_widenet_dqn_layout_query(const drl_widenet_desc* d, int32_t batch, drl_dqn_layout* layout);
int drl_widenet_dqn_init(const drl_widenet_desc* d, int32_t batch, void* d_agent, float epsilon_start,
                         hipStream_t stream);
int drl_widenet_dqn_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                          const struct drl_replay* r, int64_t size, hipStream_t stream);
int drl_widenet_dqn_sample_rows(const drl_widenet_desc* d, const drl_dqn_hparams* h, const void* d_agent,
                                int64_t size, int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Prioritized replay for the conv and the wide single-agent learners: the
 * prioritized block is drl_per_layout_query(r->capacity, h->batch)'s, filled
 * and marked by drl_per_init / drl_per_mark_new as for drl_dqn_per_train; the
 * agent blocks are the uniform learners' own (there is no new layout), so a
 * block can be handed from one call to the other.  Both calls make every
 * check of their uniform learner plus drl_dqn_per_train's (the PER
 * hyperparameters' ranges, capacity <= DRL_PER_MAX_CAPACITY, d_per 16-byte
 * aligned) before any device work, allocate nothing, do not synchronise and
 * are graph-capturable as one linear chain of kernel nodes; no workgroup
 * waits for another and no float atomic is used (the priorities' maxima are
 * integer maxima on the positive floats' bits).
 * ------------------------------------------------------------------------ */
/* drl_convnet_dqn_large_train on prioritized rows (its arguments, agent block
 * -- drl_convnet_dqn_large_layout_query / _init -- and arithmetic; batch
 * 1..4096).  With size >= h->batch, in stream order: rebuild (one or two
 * launches), sample (seed h->sample_seed, the step of the agent block's
 * counters), the rows, the dense and the conv layers' chunk partials, the
 * update, the counters, the priority update, the re-pack.  A row is
 * drl_convnet_dqn_large_train's at slot slots[b], with weights[b] = w on its
 * squared error, w * (d * d), and on the Q head's delta,
 * w * ((d + d) / float(batch)), d = q[a] - td (with w == 1.0 the row is the
 * uniform learner's bit for bit); the loss is mean(w * d^2) in the uniform
 * chain's order; |d| goes to the block's absd and the slot's leaf is zeroed.
 * The priority update is drl_dqn_per_train's: p = (float)pow((double)|d| +
 * eps, alpha), at most 2^64, the largest over the rows that drew the slot;
 * pmax = max(pmax, p).  With size < h->batch it is the uniform learner's
 * no-sample step: the tree, slots, weights and pmax are left alone.
 * alpha = 0 and beta0 = 0, beta_steps = 0 give weights and priorities of
 * exactly 1.0. */
int drl_convnet_dqn_per_train(const drl_convnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const struct drl_replay* r, int64_t size, void* d_per,
                              hipStream_t stream);
/* drl_dqn_per_train for a drl_widenet_desc (hidden widths up to
 * DRL_WIDENET_MAX_WIDTH): the same kernels on the wide family's plan, the
 * agent block drl_widenet_dqn_layout_query / _init's, then the wide pack
 * kernel.  At the widths both take, the agent block after a step is
 * drl_dqn_per_train's byte for byte. */
int drl_widenet_dqn_per_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                              void* d_agent, void* d_packed, const struct drl_replay* r, int64_t size, void* d_per,
                              hipStream_t stream);

/* ------------------------------------------------------------------------
 * A population of dense DQN agents (run_jax_sweep.py, torch_impl/sweep.py:
 * many training runs that differ in their hyperparameters): `members`
 * agents, each the learner block written above drl_dqn_train on its own
 * envs, acting and learning in the same launches.  One step of the whole
 * population is one chain of launches whose length does not depend on
 * `members`; a member's arithmetic is drl_dqn_large_train's bit for bit and
 * does not depend on which other members share the population.
 *   Envs: one batch of members * E envs; member m owns envs m*E .. m*E+E-1.
 *   Env seeding, drl_synth_actions and the exploration draw stay keyed on the
 *   global env index, so member m is reproduced by a population of one whose
 *   envs start at env_offset + m*E.
 *   Shared: the net's architecture (a drl_widenet_desc with input
 *   DRL_QNET_INPUT_CODE: a 5x5, 7x7 or 9x9 window, 1..3 hidden widths,
 *   multiples of 8 in [8, DRL_WIDENET_MAX_WIDTH], 1..8 actions), E, the ring
 *   capacity.  Per member (a drl_dqn_hparams each, uploaded once by
 *   drl_pop_init): batch in [1, max_batch], gamma, learning_rate, the Adam
 *   constants, tau, target_update_interval, the epsilon schedule,
 *   sample_seed; and the initial parameters, which the caller writes.
 * The block (device, caller-owned, 16-B aligned, drl_pop_layout.bytes):
 * `members` agent blocks member_stride bytes apart, each laid out exactly as
 * drl_dqn_large_layout_query / drl_widenet_dqn_layout_query lay out one agent
 * at batch max_batch (`member`: four parameter sets, drl_dqn_counters,
 * scratch), then the members' hyperparameter records at hparams_off.
 * The rings: a drl_replay whose five arrays hold `members` rings of
 * `capacity` rows each, ring m at row m * capacity; policy-code rows
 * (obs_floats = drl_policy_code_bytes / 4).  The cursor and size are equal
 * for every member and stay with the caller.
 * No call but drl_pop_init synchronises or reads host hyperparameters;
 * nothing is allocated, no workgroup waits for another, no float atomic is
 * used: act, add and train are graph-capturable.  Every argument is
 * validated before any device work.
 * ------------------------------------------------------------------------ */
#define DRL_POP_MAX_MEMBERS 1024
typedef struct drl_pop_layout {
    drl_dqn_layout member;   /* one member's block (offsets from the member's start) */
    int64_t member_stride;   /* bytes from member m's block to member m+1's */
    int64_t hparams_off;     /* bytes: the hyperparameter records (opaque) */
    int64_t hparams_stride;
    int64_t bytes;
    int32_t members, max_batch;
} drl_pop_layout;
/* Host only. */
int drl_pop_layout_query(const drl_widenet_desc* d, int32_t members, int32_t max_batch, drl_pop_layout* layout);
/* h, epsilon_start: HOST arrays of `members` entries.  Uploads the records
 * (synchronises `stream`), then zeroes every member's Adam moments and
 * counters on the device, epsilon = epsilon_start[m].  The caller writes the
 * online and target parameters. */
int drl_pop_init(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const drl_dqn_hparams* h,
                 const float* epsilon_start, void* d_pop, hipStream_t stream);
/* Drone 0's epsilon-greedy action of every env from its member's online f32
 * parameters (d_code: [members * E] policy-code rows; epsilon: the member's
 * device counter, or none with greedy != 0) into column 0 of d_actions
 * [members * E][n_drones], and drl_synth_actions(synth_seed, synth_step,
 * env_offset) into columns 1..n_drones-1.  The forward is f32 in the
 * learner's order, so d_q (nullable, [members * E][n_actions]) equals the
 * learner's own Q bit for bit (the MFMA acts agree with it to ~1e-5). */
int drl_pop_act(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop, const void* d_code,
                int64_t envs_per_member, int32_t greedy, uint64_t seed, uint64_t step, int64_t env_offset,
                int32_t* d_actions, int32_t n_drones, uint64_t synth_seed, uint64_t synth_step, float* d_q,
                hipStream_t stream);
/* drl_replay_add for every member: env m*E + i's drone-0 transition
 * (d_code_prev row, d_actions / d_rewards / d_dones [members * E][n_drones]
 * column 0, d_code row) lands in slot (cursor + i) % capacity of ring m; with
 * E > capacity a member's last `capacity` envs are kept.  The caller advances
 * cursor by E. */
int drl_pop_replay_add(const drl_widenet_desc* d, int32_t members, const drl_replay* r, int64_t cursor,
                       int64_t envs_per_member, const void* d_code_prev, const void* d_code, const int32_t* d_actions,
                       const float* d_rewards, const uint8_t* d_dones, int32_t n_drones, hipStream_t stream);
/* One learner step of every member on rings holding `size` rows each: member
 * m trains iff size >= its batch (decided on the device); one that does not
 * still blends its target when due, decays epsilon and advances its step. */
int drl_pop_train(const drl_widenet_desc* d, int32_t members, int32_t max_batch, void* d_pop, const drl_replay* r,
                  int64_t size, hipStream_t stream);
/* d_slots int64 [members][max_batch]: the slots member m's next step draws in
 * its first batch_m entries, -1 behind them. */
int drl_pop_sample_rows(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop, int64_t size,
                        int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Double DQN targets (van Hasselt et al. 2016) for the dense learners' launch
 * chains: an option beside the max rule, which stays the default of every
 * other call.  One step is the learner block of the corresponding max-rule
 * call (drl_dqn_large_train and the calls built on it) with one change in the
 * TD rule.  For sampled row b with A actions, all f32:
 *
 *   q  = Q_online(obs_b)        (as in the max-rule call)
 *   qs = Q_online(next_obs_b)   the online parameters the step started with,
 *                               in the chain's dot-product order (four partial
 *                               sums over k mod 4, (s0+s1)+(s2+s3), + bias; no
 *                               FMA contraction)
 *   qt = Q_target(next_obs_b)   (as in the max-rule call)
 *   a* = 0; for j = 1 .. A-1: if qs[j] > qs[a*]: a* = j
 *                               (jnp.argmax: the first maximum; a NaN never wins)
 *   td = r + (gamma * qt[a*]) * (1 - done)
 *   d  = q[a] - td
 *
 * Everything behind d is the max-rule call's: the squared error, the Q head's
 * delta (d + d) / B, the backward pass, Adam, the target blend, the counters
 * and the re-pack; a prioritized step puts the row's weight where it lies
 * there and keeps |d|.  No gradient flows through qs: the selection is an
 * index.  So (1) with the target set equal to the online set when a step
 * starts, a Double step is the max-rule step bit for bit; (2) ties resolve to
 * the lowest index; (3) the row draw, the counters, the epsilon schedule and
 * the packed image are the max-rule call's.
 *
 * The agent blocks, layouts, init calls, *_sample_rows, hyperparameter structs
 * and records are the max-rule calls' own.  The selector's forward rides in
 * the forward launches as a third grid slice and keeps its activations in the
 * scratch's delta words, so a Double step has the launches, the scratch and
 * the plan of the max-rule step.  Every argument is validated before any
 * device work with the max-rule call's checks and messages; kernel nodes
 * only, one stream, nothing allocated, nothing synchronises: graph-capturable.
 * ------------------------------------------------------------------------ */
/* drl_dqn_large_train (its arguments) with the TD rule above. */
int drl_dqn_double_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                         const struct drl_replay* r, int64_t size, hipStream_t stream);
/* drl_widenet_dqn_train (its arguments) with the TD rule above. */
int drl_widenet_dqn_double_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, void* d_agent, void* d_packed,
                                 const struct drl_replay* r, int64_t size, hipStream_t stream);
/* drl_dqn_per_train (its arguments) with the TD rule above: the row's weight
 * on w * (d * d) and w * ((d + d) / batch), |d| to the block's absd. */
int drl_dqn_double_per_train(const drl_qnet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                             void* d_agent, void* d_packed, const struct drl_replay* r, int64_t size, void* d_per,
                             hipStream_t stream);
/* drl_widenet_dqn_per_train (its arguments) with the TD rule above. */
int drl_widenet_dqn_double_per_train(const drl_widenet_desc* d, const drl_dqn_hparams* h, const drl_per_hparams* ph,
                                     void* d_agent, void* d_packed, const struct drl_replay* r, int64_t size,
                                     void* d_per, hipStream_t stream);
/* drl_pop_train with the rule chosen per member: d_double is a DEVICE array of
 * `members` bytes, nonzero = member m's TD rule is the one above, 0 = the max
 * rule (the member's selector slice returns at once).  With every byte 0 the
 * population block is left byte for byte as drl_pop_train leaves it. */
int drl_pop_double_train(const drl_widenet_desc* d, int32_t members, int32_t max_batch, void* d_pop,
                         const drl_replay* r, int64_t size, const uint8_t* d_double /* DEVICE [members] */,
                         hipStream_t stream);

/* ------------------------------------------------------------------------
 * Prioritized replay for a population of dense DQN agents: every member
 * owns a priority tree over its ring and its own drl_per_hparams (alpha,
 * beta0, beta_steps, eps), so one population sweeps them.  The members
 * sample, train and write their priorities back in the population's chain:
 * the launch count of a step does not depend on `members`.  A member's
 * arithmetic is drl_dqn_per_train's bit for bit at the widths both take (the
 * same device bodies: rebuild, the stratified draw written above
 * drl_per_sample with the member's batch, sample_seed, its own counter's step
 * and its record's beta, the weighted TD error, the priority update) and does
 * not depend on which other members share the population.  The description,
 * the population block, the rings, drl_pop_act and drl_pop_replay_add are
 * drl_pop_*'s, unchanged; hidden widths up to DRL_WIDENET_MAX_WIDTH.
 *   The block (device, caller-owned, 16-B aligned, drl_pop_per_layout.bytes):
 *   `members` prioritized blocks member_stride bytes apart, each laid out
 *   exactly as drl_per_layout_query(capacity, max_batch) lays out one agent
 *   (`member`: tree[2P], pmax, wmax, slots, weights, |d|; member m uses the
 *   first batch_m entries of the three arrays), then one record of PER
 *   hyperparameters per member at hparams_off.  The rings, the cursor and the
 *   size are the population's: one cursor and one size for all members.
 *   A member trains iff size >= its batch (decided on the device).  One that
 *   does not is skipped by rebuild, sample and the chain up to the backward:
 *   its tree, pmax, slots and weights are left alone, as drl_dqn_per_train
 *   leaves them; it still blends its target when due, decays epsilon and
 *   advances its step.
 * No call but drl_pop_per_init synchronises or reads host hyperparameters;
 * nothing is allocated, no workgroup waits for another, no float atomic is
 * used: mark, rebuild, sample and train are graph-capturable.  Every argument
 * is validated before any device work.
 * ------------------------------------------------------------------------ */
typedef struct drl_pop_per_layout {
    drl_per_layout member;   /* one member's block (offsets from the member's start) */
    int64_t member_stride;   /* bytes from member m's block to member m+1's */
    int64_t hparams_off;     /* bytes: the PER records (opaque) */
    int64_t hparams_stride;
    int64_t bytes;
    int32_t members, max_batch;
} drl_pop_per_layout;
/* Host only.  members in [1, DRL_POP_MAX_MEMBERS], capacity in [1, DRL_PER_MAX_CAPACITY], max_batch in
 * [1, DRL_DQN_LARGE_MAX_BATCH]. */
int drl_pop_per_layout_query(int32_t members, int64_t capacity, int32_t max_batch, drl_pop_per_layout* layout);
/* ph: a HOST array of `members` drl_per_hparams (drl_per_hparams' ranges).  Uploads the records (synchronises
 * `stream`), then zeroes every member's tree, pmax = 1. */
int drl_pop_per_init(int32_t members, int64_t capacity, int32_t max_batch, const drl_per_hparams* ph, void* d_pper,
                     hipStream_t stream);
/* After drl_pop_replay_add with the same cursor and count = envs_per_member: the leaves of slots
 * [cursor, cursor + count) mod capacity of every member = that member's own pmax (count > capacity marks every
 * slot). */
int drl_pop_per_mark_new(int32_t members, int64_t capacity, int32_t max_batch, void* d_pper, int64_t cursor,
                         int64_t count, hipStream_t stream);
/* Every internal node of every member's tree from its leaves (two launches at most). */
int drl_pop_per_rebuild(int32_t members, int64_t capacity, int32_t max_batch, void* d_pper, hipStream_t stream);
/* drl_per_sample for every member with size >= its batch, from rebuilt trees with positive roots: the member's
 * slots, weights (its first batch_m entries; the rest untouched) and wmax for the step its own counters hold.
 * size in [1, capacity]. */
int drl_pop_per_sample(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop, void* d_pper,
                       int64_t capacity, int64_t size, hipStream_t stream);
/* drl_pop_train on prioritized rows (its arguments; d_pper laid out for (members, r->capacity, max_batch)): one
 * drl_dqn_per_train step of every member without the re-pack -- rebuild, sample, the rows at the drawn slots,
 * each layer's forward of both nets, the weighted TD error, the priority update into the member's leaves and
 * pmax, each layer's backward, the update (with the target blend of members that do not train), the counters. */
int drl_pop_per_train(const drl_widenet_desc* d, int32_t members, int32_t max_batch, void* d_pop, const drl_replay* r,
                      int64_t size, void* d_pper, hipStream_t stream);

/* ------------------------------------------------------------------------
 * A population of conv DQN agents (run_jax_sweep.py draws network_type from
 * ['dense', 'conv']): the five drl_pop_* calls above for a drl_convnet_desc
 * with input DRL_QNET_INPUT_CODE (a 5x5, 7x7 or 9x9 window; every other
 * limit is drl_convnet_dqn_large_*'s).  Each member is the learner block
 * written above drl_convnet_dqn_train on its own envs; a member's arithmetic
 * is drl_convnet_dqn_large_train's bit for bit and does not depend on which
 * other members share the population; one step of all members is one chain
 * of launches whose length does not depend on `members` (rows, the dense and
 * the conv layers' chunk partials, update, counters).
 *   Envs, what is shared and what a member owns: as for drl_pop_*.
 *   The block: `members` agent blocks member_stride bytes apart, each laid
 *   out exactly as drl_convnet_dqn_large_layout_query lays out one agent at
 *   batch max_batch, then the hyperparameter records at hparams_off.
 *   The rings: drl_pop_replay_add's, unchanged (it reads the window alone of
 *   its description: pass a drl_widenet_desc with in_features = W*W*6).
 *   The act is an f32 forward on the member's online set by the learner's
 *   own per-layer code, one workgroup per env: its Q is the learner's Q bit
 *   for bit.  There is no packed image and nothing is re-packed after a
 *   train step.  drl_convnet_act (MFMA) agrees with it to ~1e-5, not bit for
 *   bit: a member reproduces under this API, not necessarily under the
 *   single-agent calls.
 * No call but drl_convpop_init synchronises or reads host hyperparameters;
 * nothing is allocated, no workgroup waits for another, no float atomic is
 * used: act and train are graph-capturable.  Every argument is validated
 * before any device work.
 * ------------------------------------------------------------------------ */
typedef struct drl_convpop_layout {
    drl_convnet_dqn_layout member; /* one member's block (offsets from the member's start) */
    int64_t member_stride;         /* bytes from member m's block to member m+1's */
    int64_t hparams_off;           /* bytes: the hyperparameter records (opaque) */
    int64_t hparams_stride;
    int64_t bytes;
    int32_t members, max_batch;    /* 1..DRL_POP_MAX_MEMBERS; 1..DRL_CONVNET_DQN_LARGE_MAX_BATCH */
} drl_convpop_layout;
/* Host only. */
int drl_convpop_layout_query(const drl_convnet_desc* d, int32_t members, int32_t max_batch, drl_convpop_layout* layout);
/* drl_pop_init's arguments and effects (the only call that synchronises). */
int drl_convpop_init(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const drl_dqn_hparams* h,
                     const float* epsilon_start, void* d_pop, hipStream_t stream);
/* drl_pop_act's arguments and rule. */
int drl_convpop_act(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop, const void* d_code,
                    int64_t envs_per_member, int32_t greedy, uint64_t seed, uint64_t step, int64_t env_offset,
                    int32_t* d_actions, int32_t n_drones, uint64_t synth_seed, uint64_t synth_step, float* d_q,
                    hipStream_t stream);
/* drl_pop_train's arguments and rule. */
int drl_convpop_train(const drl_convnet_desc* d, int32_t members, int32_t max_batch, void* d_pop, const drl_replay* r,
                      int64_t size, hipStream_t stream);
/* drl_pop_sample_rows' arguments and result. */
int drl_convpop_sample_rows(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                            int64_t size, int64_t* d_slots, hipStream_t stream);

/* ------------------------------------------------------------------------
 * A league (torch_impl/helpers/rl_helpers.py MultiAgentTrainer.train): K
 * learners that share ONE batch of E envs, learner k driving drone INDEX k
 * of every env and learning from that drone's transitions.  Each learner is
 * exactly a population member: the block is drl_pop_layout_query's with
 * members = K, initialised by drl_pop_init, trained by drl_pop_train and
 * sampled by drl_pop_sample_rows, all unchanged; the rings are the
 * population's (K rings of `capacity` policy-code rows, ring k at row
 * k * capacity, one cursor and size for all, advanced by E per step).
 * 1 <= members <= min(n_drones, DRL_POP_MAX_MEMBERS).  Drones K..N-1 are the
 * caller's (drl_synth_actions, or fixed nets through the code acts).
 * The codes are drl_obs_code_all's output, [n_drones][E][code bytes]; learner
 * k reads block k.  Neither call allocates or synchronises; no workgroup
 * waits for another and no float atomic is used: both are graph-capturable.
 * Every argument is validated before any device work.
 * ------------------------------------------------------------------------ */
typedef struct drl_league_act_plan {
    int32_t env_tile;    /* envs of one learner a workgroup takes through every layer */
    int32_t threads;     /* its size */
    int32_t pass_units;  /* units of a layer it computes per pass over the inputs */
    int32_t chunk_k;     /* input columns of a staged weight chunk */
    int32_t ldx, lda;    /* LDS row strides (floats): decoded inputs, activations */
    int32_t lds_bytes;   /* dynamic LDS of the launch */
    int32_t lds_limit;   /* what lds_bytes stays within (a CU's 160 KiB) */
} drl_league_act_plan;
/* Host only: the act's tiling for a population description. */
int drl_league_act_plan_query(const drl_widenet_desc* d, drl_league_act_plan* plan);
/* Learner k's epsilon-greedy action of env i from its online f32 parameters
 * on d_codes block k, into d_actions[i * n_drones + k] for k < members and NO
 * other column.  The exploration draw is the population's with the stream
 * seed + k (mod 2^64): explore_draw(seed + k, step, env_offset + i,
 * n_actions, epsilon_k), epsilon_k the learner's device counter, or none with
 * greedy != 0; with k = 0 this is drl_pop_act's stream.  The forward is f32
 * in the learner's order (four partial sums over k mod 4, (s0 + s1) +
 * (s2 + s3), + bias, nothing contracted), so d_q (nullable, [members][E]
 * [n_actions]) equals the learner's own Q bit for bit. */
int drl_league_act(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                   const void* d_codes, int64_t num_envs, int32_t greedy, uint64_t seed, uint64_t step,
                   int64_t env_offset, int32_t* d_actions, int32_t n_drones, float* d_q, hipStream_t stream);
/* Ring k, slot (cursor + i) % capacity, receives d_codes_prev[k][i],
 * d_actions / d_rewards / d_dones [i][k] and d_codes[k][i]; with E > capacity
 * the last `capacity` envs are kept (drl_pop_replay_add's rule).  The caller
 * advances cursor by E. */
int drl_league_replay_add(const drl_widenet_desc* d, int32_t members, const drl_replay* r, int64_t cursor,
                          int64_t num_envs, const void* d_codes_prev, const void* d_codes, const int32_t* d_actions,
                          const float* d_rewards, const uint8_t* d_dones, int32_t n_drones, hipStream_t stream);

/* ------------------------------------------------------------------------
 * A league of conv learners: the same league with every learner a member of a
 * drl_convpop_layout block (members = K), initialised by drl_convpop_init,
 * trained by drl_convpop_train and sampled by drl_convpop_sample_rows, all
 * unchanged; the rings are the population's and drl_league_replay_add feeds
 * them (it reads the code window and the member count of its description
 * alone).  Only the act is new: drl_convpop_act's workgroup takes one env and
 * fetches the member's weights once per env; a league has few learners with
 * thousands of envs each, so here a workgroup takes env_tile envs of one
 * learner through every layer and each weight word it fetches serves them all.
 * The call neither allocates nor synchronises; no workgroup waits for another
 * and no float atomic is used: it is graph-capturable.  Every argument is
 * validated before any device work.
 * ------------------------------------------------------------------------ */
typedef struct drl_convleague_act_plan {
    int32_t env_tile;   /* envs of one learner a workgroup takes through every layer (16, 8, 4 or 2) */
    int32_t threads;    /* its size */
    int32_t row_words;  /* LDS words of an env's forward-only row: input, every layer's output */
    int32_t lds_bytes;  /* dynamic LDS of the launch: env_tile * row_words * 4 */
    int32_t lds_limit;  /* what lds_bytes stays within (a CU's 160 KiB) */
} drl_convleague_act_plan;
/* Host only: the act's tiling for a conv population description. */
int drl_convleague_act_plan_query(const drl_convnet_desc* d, drl_convleague_act_plan* plan);
/* drl_league_act's arguments, rule and streams for a conv population block:
 * learner k's action of env i into d_actions[i * n_drones + k] for k < members
 * and NO other column, its draw explore_draw(seed + k, step, env_offset + i,
 * n_actions, epsilon_k).  The forward is the conv learner's own per-row
 * forward (drl_convpop_act's: taps in (ci, ky, kx) order, a dense unit's 64
 * partial sums and xor tree, nothing contracted), so d_q (nullable,
 * [members][E][n_actions]) equals drl_convpop_act's Q bit for bit. */
int drl_convleague_act(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                       const void* d_codes, int64_t num_envs, int32_t greedy, uint64_t seed, uint64_t step,
                       int64_t env_offset, int32_t* d_actions, int32_t n_drones, float* d_q, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Shared-policy self-play (MultiAgentTrainer.train with one agent object
 * under several keys of its `agents` dict): K learners that share ONE batch
 * of E envs, learner k driving the `team` drone indices drones[k][0..team-1]
 * of every env and learning from all of their transitions into its one ring.
 * `drones` is a HOST array [members][team] of distinct indices in
 * [0, n_drones), members * team <= n_drones; it travels to the kernels by
 * value.  Each learner is exactly a population member, as in the league: the
 * block, drl_pop_init, drl_pop_train and drl_pop_sample_rows are unchanged,
 * the rings are the population's (one cursor and size for all, advanced by
 * team * E per step: every learner drives the same number of drones).
 * Drones in no team are the caller's.  A learner's rows are its team * E
 * (drone, env) pairs taken slot-major, r = j * E + i.  The act's tiling is
 * drl_league_act_plan_query's with a tile of env_tile consecutive rows r.
 * Neither call reads device memory on the host, allocates or synchronises;
 * no workgroup waits for another and no float atomic is used: both are
 * graph-capturable.  Every argument is validated before any device work.
 * ------------------------------------------------------------------------ */
/* For learner k, team slot j and env i, with dr = drones[k][j]: the
 * epsilon-greedy action from the learner's online f32 parameters on
 * d_codes[dr][i], into d_actions[i * n_drones + dr] and NO column outside the
 * teams.  The draw is explore_draw(seed + dr, step, env_offset + i,
 * n_actions, epsilon_k), epsilon_k the learner's device counter, or none with
 * greedy != 0: the stream is keyed on the drone index, so two drones of a
 * team never share one.  The forward is drl_league_act's (four partial sums
 * over k mod 4, (s0 + s1) + (s2 + s3), + bias, nothing contracted); d_q is
 * nullable, [members][team][E][n_actions].  With team = 1 and
 * drones[k][0] = k the actions and d_q are drl_league_act's byte for byte. */
int drl_selfplay_act(const drl_widenet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                     const void* d_codes, int64_t num_envs, const int32_t* drones /* HOST [members][team] */,
                     int32_t team, int32_t greedy, uint64_t seed, uint64_t step, int64_t env_offset,
                     int32_t* d_actions, int32_t n_drones, float* d_q, hipStream_t stream);
/* Ring k, slot (cursor + j * E + i) % capacity, receives d_codes_prev[dr][i],
 * d_actions / d_rewards / d_dones [i][dr] and d_codes[dr][i]; with
 * team * E > capacity only the rows with j * E + i >= team * E - capacity are
 * stored (ReplayBuffer.add_many on the team's rows taken slot-major).  The
 * caller advances cursor by team * E. */
int drl_selfplay_replay_add(const drl_widenet_desc* d, int32_t members, const drl_replay* r, int64_t cursor,
                            int64_t num_envs, const int32_t* drones, int32_t team, const void* d_codes_prev,
                            const void* d_codes, const int32_t* d_actions, const float* d_rewards,
                            const uint8_t* d_dones, int32_t n_drones, hipStream_t stream);
/* drl_selfplay_act's arguments, rule and streams for learners that are
 * members of a drl_convpop_layout block (initialised by drl_convpop_init,
 * trained by drl_convpop_train, sampled by drl_convpop_sample_rows; the rings
 * are fed by drl_selfplay_replay_add, which reads the code window and the
 * member count of its description alone).  For learner k, team slot j and env
 * i, with dr = drones[k][j]: the action of the learner's online set on
 * d_codes[dr][i] into d_actions[i * n_drones + dr] and NO column outside the
 * teams, its draw explore_draw(seed + dr, step, env_offset + i, n_actions,
 * epsilon_k), or none with greedy != 0.  The forward is the conv learner's
 * own per-row forward (drl_convpop_act's: taps in (ci, ky, kx) order, a dense
 * unit's 64 partial sums and xor tree, nothing contracted); d_q is nullable,
 * [members][team][E][n_actions].  The tiling is drl_convleague_act_plan_query's
 * with a tile of env_tile consecutive rows r = j * E + i of one learner
 * (team * num_envs < 2^31).  With team = 1 and drones[k][0] = k the actions
 * and d_q are drl_convleague_act's byte for byte.  Graph-capturable, as both
 * of those calls. */
int drl_convselfplay_act(const drl_convnet_desc* d, int32_t members, int32_t max_batch, const void* d_pop,
                         const void* d_codes, int64_t num_envs, const int32_t* drones /* HOST [members][team] */,
                         int32_t team, int32_t greedy, uint64_t seed, uint64_t step, int64_t env_offset,
                         int32_t* d_actions, int32_t n_drones, float* d_q, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRONERL_H */
