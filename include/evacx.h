/* evacx -- C-ABI of the MI355X-native evacuation CA + DQN hot path (libevacx.so).
 *
 * The reference (LX-530/DQN-MARL, Louvre_Evacuation/) has no FFI: its boundary
 * is the duck-typed Python API its runners call. Each entry point below names
 * the reference function it replaces (paths relative to
 * /root/reference/Louvre_Evacuation/); the Python mirror in
 * dqn-marl_amd/Louvre_Evacuation binds them through ctypes.
 *
 * Conventions
 *  - every call returns 0 or a negative errno-like code; evx_last_error() has text: the message
 *    of the calling thread's last failed call (the evx_*_last_error getters return the same buffer);
 *  - every buffer is caller-owned DEVICE memory unless the name says _host;
 *  - no hidden allocations, no internal threads, no host syncs; `stream` is a
 *    hipStream_t passed as void* (0 = the null stream);
 *  - plain pointers and sizes only (no torch types).
 */
#ifndef EVACX_H
#define EVACX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVX_MT_WORDS 625 /* 624 MT19937 words + index, CPython/numpy layout */
#define EVX_OBS_CELLS 121
#define EVX_OBS_CH 6

/* Static, read-only description of one layout (device tables built on the host
 * by evacx/layout.py: Map.__init__ + Init_Potential envs/map.py:38-148,
 * ProgressiveFireModel envs/fire_model.py:4-199). */
typedef struct {
    int32_t L, W;             /* interior; padded grid (L+2)x(W+2), cell = x*(W+2)+y */
    int32_t P, R;             /* people per env, robots per env */
    int32_t t_max;            /* fire max_steps (tables hold t = 0..t_max) */
    int32_t ox0, oy0, OX, OY; /* danger_o window origin / size */
    int32_t exit_x, exit_y;   /* EvacuationEnv.exit_location */
    int32_t rx_lo, rx_hi;     /* Map.robot_range (envs/map.py:75) */
    int32_t reset_view_x, reset_view_y; /* Map.robot_position set by reset (envs/evacuation_env.py:64) */
    int32_t reset_robots;     /* 1 = EvacuationEnvMulti.reset re-places robots */
    int32_t flags;            /* EVX_LAYOUT_* */
    int32_t repel_d2;         /* smallest integer n with sqrt(n) >= repel_range (host-computed) */
    int32_t pad0;
    double repel_k, repel_range;  /* People.ROBOT_REPEL_K / _RANGE (envs/people.py:94-95) */
    double evac_reward, death_penalty, death_acc_penalty, alive_bonus; /* envs/evacuation_env.py:16-19 */
    const double *floor;      /* [G] floor field */
    const uint8_t *cellinfo;  /* [G] bit0 valid, bit1 exit (checkSavefy), bit2 barrier_list */
    const uint32_t *valid_bits; /* [ceil(G/32)] bit0 of cellinfo as a bitmap */
    const double *danger_p;   /* [(t_max+1)*G] danger at person positions (x+.5,y+.5) */
    const double *danger_o;   /* [(t_max+1)*OX*OY] danger at integer obs coordinates */
    const float *danger_o32;  /* same, float32 (network input path) */
    const int32_t *robot_init;/* [R*2] robot positions after a multi-robot reset */
    const uint8_t *nbr_valid; /* [G] bit d: Check_Valid of the MoveTO[d] neighbour (envs/people.py:259-265) */
    const double *floor_d5;   /* [G][8] (floor[c] - floor[c + MoveTO[d]]) * 5.0 = getDeltaP * 5.0 (envs/people.py:268,282) */
    /* [(t_max+1)][L+2+2*EVX_FEAT_PAD][W+2+2*EVX_FEAT_PAD] static observation features of map
     * cell (x, y) at index (t, x + PAD, y + PAD): bf16(danger_o32) in bits 0-15, the
     * barrier channel (!valid || barrier_list) in bit 16, the exit channel in bit 17
     * (_get_state's channels 2-4, envs/evacuation_env.py:84-120); read by the MLP fast path */
    const uint32_t *obs_feat;
    /* Layout set (per-env layouts), or NULL: a device array of the evx_layout
     * descriptors of every layout of the set -- all of one size (L, W, P, R, t_max, OX, OY) --
     * indexed by evx_state.layout_idx[e] in the env kernels and by evx_obs.layout in the
     * observation readers; obs_feats is the device array of their obs_feat tables. */
    const void *layout_set;
    const uint32_t *const *obs_feats;
    /* f32-accurate MLP inputs (evx_qmlp_params.x3): the bf16 residual of the danger feature,
     * bf16(danger_o32 - bf16(danger_o32)), indexed as obs_feat; obs_feats_lo: per layout of a set */
    const uint16_t *obs_feat_lo;
    const uint16_t *const *obs_feats_lo;
} evx_layout;

#define EVX_FEAT_PAD 6

/* Structure-of-arrays state of E env instances (env-major). */
typedef struct {
    int32_t E;
    uint32_t *pk;      /* [E*P] person: x | y<<12 | safe<<24 | dead<<25 */
    double *health;    /* [E*P] Person.health */
    double *acc;       /* [E*P] Person.move_accumulator */
    uint32_t *rmap;    /* [E*ceil(G/32)] People.rmap as a bitmap */
    int32_t *thmap;    /* [E*G] People.thmap, or NULL (diagnostic heat map) */
    uint32_t *robots;  /* [E*R] Map.robot_positions: (uint16)x | (uint16)y<<16 */
    uint32_t *view;    /* [E]   Map.robot_position (same packing) */
    int32_t *scal;     /* [E*4] fire_step, current_step, prev_evacuated, prev_dead */
    uint32_t *py_mt;   /* [E*625] CPython `random` MT19937 state per env */
    uint32_t *np_mt;   /* [E*625] legacy numpy.random MT19937 state per env */
    uint32_t *scratch; /* [E*evx_step_scratch_words] step scratch: move plan, contested lists beyond LDS */
    int32_t *order;    /* [E+1] dispatch order of the step's envs (evx_env_order), or NULL = 0..E-1;
                        * order[E] = H: the first H of them are heavy (rows phase on a 4-wave workgroup) */
    const int32_t *layout_idx; /* [E] each env's layout in evx_layout.layout_set, or NULL (one layout) */
    uint8_t *perm_ws;  /* [evx_perm_ws_bytes(E)] one class byte per env for the scheduling
                        * permutations (persons-remaining bucket, fire step >= t_max, heavy),
                        * written by the step and reset kernels as they finish an env (or by
                        * evx_env_classes from the state words) and read by evx_env_order /
                        * evx_act_perm / evx_env_orders, one launch each. NULL: evx_env_order
                        * reads the state words itself, evx_act_perm / evx_env_orders fail */
} evx_state;

/* Compact per-robot observation (32 B). Expands to the reference's 11x11x6
 * _get_state tensor (envs/evacuation_env.py:84-120) given the layout. */
typedef struct {
    uint32_t occ[4];   /* bit c (c = i*11+j): People.rmap at (cx+i-5, cy+j-5) if valid */
    int32_t cx, cy;    /* window centre */
    int32_t fire_step; /* env fire model step the obs was taken at */
    int32_t layout;    /* the env's layout in evx_layout.layout_set (0 without a set) */
} evx_obs;

/* Per-step outputs. */
typedef struct {
    double *reward;    /* [E] EvacuationEnv._calculate_reward (envs/evacuation_env.py:174-288) */
    uint8_t *done;     /* [E] */
    int32_t *counts;   /* [E*2] evacuated, dead after the step (may be NULL) */
    evx_obs *obs;      /* [E*R] observation after the step */
    int32_t *err;      /* [1] sticky device error word (may be NULL); bits: 1 > 128 movers on one
                        * target, 2 a runaway Python-stream window, 4 reset placement, 8 / 16
                        * scratch overflow / more than 256 order-sensitive events on one cell (more
                        * events than the LDS list holds over a whole step are handled: the plan is
                        * walked again per range of cells), 32 kept-list mismatch, 64 an MT block
                        * overwritten before the state store (any bit: results not bit-exact) */
    int64_t *stamps;   /* [E*48] diagnostic per-phase s_memtime stamps + counters (NULL = off) */
    /* Auto-reset (NULL = off, the reference's separate env.reset): envs that finish this
     * step are reset in the same launch (evx_env_reset semantics); their terminal
     * observations go to obs_term [E*R] and obs receives the post-reset ones. */
    evx_obs *obs_term;
} evx_step_out;

/* Replaces EvacuationEnv.step / EvacuationEnvMulti.step (envs/evacuation_env.py:122-172,
 * envs/evacuation_env_multi.py:55-89): robot moves (Map.move_robot envs/map.py:160-201),
 * People.run (envs/people.py:196-314), fire update, reward, counters, observation.
 * actions: [E*R] int32; values outside 0..4 are ignored as in the reference. */
int evx_env_step(const evx_layout *lay, const evx_state *st, const int32_t *actions,
                 const evx_step_out *out, void *stream);
/* The same step in two launches that may run concurrently on two streams: part 1 steps the
 * heavy envs of the dispatch order (order[0, order[E]), one workgroup each), part 2 every
 * other env; part 0 = evx_env_step. Both parts of one step must be launched with the same
 * state, order, actions and outputs; results are identical to the one-launch step. */
int evx_env_step_part(const evx_layout *l, const evx_state *s, const int32_t *actions, const evx_step_out *o,
                      int32_t part, void *stream);
/* Diagnostics, launches nothing: the workgroup evx_env_step_part would launch for this layout and
 * st->E (only E, order and layout_idx of st are looked at, none dereferenced) -- its threads, its
 * dynamic LDS bytes, and how many such workgroups the runtime says one CU holds
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor: registers, LDS allocation granule, wave slots).
 * EVX_ENV_NWB = 1 / 2 / 4 in the environment overrides the waves per workgroup of both. */
int evx_env_step_occupancy(const evx_layout *l, const evx_state *s, int32_t *blocks_per_cu, int32_t *lds_bytes,
                           int32_t *block_threads);
/* How a step of st->E envs of this layout is launched: env_step_kernel<nwb, multi, bigg>, its LDS and
 * the heavy-env path, with the three places where the LDS layout of an env switches. */
typedef struct {
    int32_t nwb;            /* waves (envs) per workgroup: 1, 2 or 4. 4 below 64 envs per CU (big grids: 2
                             * below 32), else 1; EVX_ENV_NWB = 1 / 2 / 4 overrides; halved while the
                             * workgroup's LDS exceeds 160 KiB */
    int32_t bigg;           /* 1: a big grid (bitmaps of more than 1024 words: target / contested / vacated
                             * bitmaps in the env's global scratch, no heavy path, nwb <= 2) */
    int32_t multi;          /* 1: per-env layouts (evx_layout.layout_set with evx_state.layout_idx) */
    int32_t hcap;           /* most heavy envs (rows phase on a 4-wave workgroup) per step; 0: none -- nwb < 4,
                             * no order buffer, a big grid, or the 4-wave workgroup does not fit 160 KiB
                             * (EVX_HEAVY_CAP overrides, read once per process) */
    int32_t hmin;           /* persons in play that make an env heavy: max(1, P / 4) (EVX_HEAVY_MIN
                             * overrides, read once per process); 0 when nwb < 4 or without an order buffer */
    int32_t lds_env_bytes;  /* dynamic LDS of one env's wave (evx_step_lds_bytes) */
    int32_t lds_wg_bytes;   /* dynamic LDS of the workgroup */
    int32_t vac_in_ring;    /* 1: the vacated-cell bitmap overlays the Python MT ring (bitmaps of <= 624
                             * words); 0: a region of its own, or (big grids) global scratch */
    int32_t near_in_misc;   /* 1: the near-robot block map overlays the shuffle-group region (<= 144 words:
                             * grids up to 266 x 266); 0: a region of its own */
    int32_t wide_past_envs; /* 1: the heavy path's rows buffers run past the four env regions of the
                             * 4-wave workgroup (0 on big grids, which have no heavy path) */
} evx_env_step_plan;
/* The plan evx_env_step_part launches by, from the function the launcher itself switches on. ncu > 0:
 * the compute units to plan for -- no device call at all, so it runs on a host without a GPU;
 * ncu <= 0: the current device's. Only E, order and layout_idx of st are looked at, none
 * dereferenced, and no table of the layout is read. An argument error the step would report
 * before launching comes back as the same code with the same evx_last_error text. */
int evx_env_step_plan_query(const evx_layout *l, const evx_state *s, int32_t ncu, evx_env_step_plan *out);

/* Replaces EvacuationEnv.reset / EvacuationEnvMulti.reset (envs/evacuation_env.py:61-82,
 * envs/evacuation_env_multi.py:31-42) incl. People placement (envs/people.py:183-194).
 * mask: [E] uint8 (NULL = all envs); obs receives the reset observation of masked envs. */
int evx_env_reset(const evx_layout *lay, const evx_state *st, const uint8_t *mask, evx_obs *obs,
                  int32_t *err, void *stream);

/* Expands n compact observations to the reference tensor layout [n][11][11][6]. */
int evx_obs_expand_f32(const evx_layout *lay, const evx_obs *obs, int64_t n, float *out, void *stream);
int evx_obs_expand_f64(const evx_layout *lay, const evx_obs *obs, int64_t n, double *out, void *stream);

/* Host helper: MT19937 states for integer seeds as random.seed(s) (init_by_array)
 * and numpy.random.seed(s) (init_genrand) produce them. Host pointers. */
int evx_seed_host(const uint32_t *seeds_host, int32_t n, uint32_t *py_mt_host, uint32_t *np_mt_host);

/* Scheduling only (results do not depend on it): st->order = envs by descending
 * persons still in play, so the heaviest env-steps start first; order[E] = how many
 * of the first get a whole workgroup each (at most 256, each with >= P/4 persons in
 * play; EVX_HEAVY_CAP / EVX_HEAVY_MIN override). */
int evx_env_order(const evx_layout *lay, const evx_state *st, void *stream);
/* act row permutation for the x3 act fast path: perm[0..E) lists the envs whose fire step is >= the
 * layout's t_max (the static-table fire step) first, then the rest, each in env order (stable) */
int evx_act_perm(const evx_layout *l, const evx_state *s, int32_t *perm, void *stream);
/* Both of the above in one launch: st->order for the next step and perm for the
 * next act, from the class bytes the step just wrote. */
int evx_env_orders(const evx_layout *l, const evx_state *s, int32_t *perm, void *stream);
/* Rewrites every env's class byte in st->perm_ws from st->scal (a state written from the host). */
int evx_env_classes(const evx_layout *l, const evx_state *s, void *stream);
/* Bytes of evx_state.perm_ws for E envs. */
int64_t evx_perm_ws_bytes(int32_t E);

/* Bytes of dynamic LDS the step kernel needs for a layout (diagnostics). */
int64_t evx_step_lds_bytes(const evx_layout *lay);
/* 32-bit words of evx_state.scratch the step needs per env. */
int64_t evx_step_scratch_words(const evx_layout *lay);
/* Test entry (no reference counterpart): one wave sorts keys[0..n) (distinct u32) in place with
 * the step's contested-list sort (envs/people.py:284-297 groups movers by target through it);
 * pad: device scratch of the next power of two >= n words. */
int evx_diag_sort_keys(uint32_t *keys, uint32_t *pad, int32_t n, void *stream);

const char *evx_last_error(void);

/* ------------------------------------------------------------------ learner
 * DQNNetwork / DQNAgent (agents/dqn_agent.py:15-191) as device primitives. */

#define EVX_PREC_F32 0   /* exact f32 MFMA (v_mfma_f32_32x32x2_f32), parity path */
#define EVX_PREC_BF16 1  /* bf16 inputs, f32 accumulate (v_mfma_f32_32x32x16_bf16) */
#define EVX_PREC_X3 2    /* f32-accurate: bf16 hi + lo operand pairs, hi*hi + hi*lo + lo*hi on the bf16 MFMA */
#define EVX_GEMM_RELU 1
#define EVX_GEMM_ACCUM 2
/* X3 only. SPLIT_AB: A and B hold bf16 hi / lo planes (k-contiguous: sak = sbk = 1; A's lo plane
 * M*sam elements after its hi plane, B's N*sbn after) -- their staging copies 16-B pieces instead
 * of splitting f32 per element. OUT_SPLIT (evx_conv3x3_gemm forward, LDS-staged kernel only): C is
 * written as bf16 hi / lo planes, the lo plane M*ldc elements after the hi plane. */
#define EVX_GEMM_SPLIT_AB 4
#define EVX_GEMM_OUT_SPLIT 8

/* C[m][n] = epi(alpha * sum_k A(m,k) B(k,n) + bias[n]) with A(m,k) = A[m*sam + k*sak],
 * B(k,n) = B[k*sbk + n*sbn], C[m*ldc + n]; epilogue order: bias, ReLU, dropout mask
 * (mask[m*ldm+n] ? v*mask_scale : 0), ReLU-backward gate (gate[m*ldg+n] > 0 ? v : 0),
 * accumulate. Covers nn.Linear forward (A x W^T), its dX (dY W) and dW (dY^T X).
 * BF16 / X3 GEMMs with a long K and few 128x128 tiles (fewer than 256 without an epilogue, at
 * most 256 with one) may be split over K when the caller passes a workspace: each K slice
 * stores its raw partial into ws[z][M][N] and a second launch on the same stream adds the
 * slices in slice order and applies the epilogue (deterministic: the same bits on every call).
 * The slice count is capped by ws_elems / (M*N); ws = NULL runs the GEMM in one pass.
 * evx_gemm_ws_elems gives the workspace a descriptor's full split uses (0: never split).
 * EVX_PREC_F32 never splits. */
typedef struct {
    int32_t M, N, K;
    int32_t precision;         /* EVX_PREC_* */
    int32_t flags;             /* EVX_GEMM_* */
    float alpha;
    const float *A; int64_t sam, sak;
    const float *B; int64_t sbk, sbn;
    float *C; int64_t ldc;
    const float *bias;         /* [N] or NULL */
    const uint8_t *mask; int64_t ldm; float mask_scale;  /* or NULL */
    const float *gate; int64_t ldg;                        /* or NULL */
    float *ws; int64_t ws_elems;  /* split-K workspace (f32 elements) or NULL */
} evx_gemm_desc;

typedef struct {
    float lr, beta1, beta2, eps, weight_decay;
    int64_t step;  /* 1-based step count after increment (torch.optim.Adam state['step']) */
} evx_adam;

/* Uniform replay ring of compact observations (DQNAgent.memory, agents/dqn_agent.py:88-99). */
typedef struct {
    int64_t capacity;
    evx_obs *s, *s2;
    int32_t *a;
    float *r;
    uint8_t *done;
} evx_replay;

int evx_gemm(const evx_gemm_desc *g, void *stream);
int64_t evx_gemm_ws_elems(const evx_gemm_desc *g);
/* Implicit-GEMM 3x3 convolution, padding 1, on 11x11 maps (DQNNetwork conv1-3,
 * agents/dqn_agent.py:22-24,48-50, in place of im2col + evx_gemm; x3 precision only). The
 * activations are pixel-major [B*121][cs]; the operand they feed is gathered in the tile fetch:
 *   EVX_CONV_FWD: C[m][n] = sum_{tap,c} A[m shifted by tap][c] W[n][c][tap]; M = B*121, K = 9 cs,
 *                 B = W with sbk = 9 (c stride), sbn = 9 cs (n stride). Epilogue as evx_gemm.
 *   EVX_CONV_DX:  C[m][n] = sum_{tap,o} A[m shifted by -tap][o] W[o][n][tap] (dX of the layer,
 *                 A = dY [B*121][cs]); K = 9 cs, B = W with sbk = 9 N, sbn = 9; gate = the
 *                 layer input (ReLU backward of the layer below).
 *   EVX_CONV_DW:  C[o][c*9+tap] = sum_m A[m][o] B[m shifted by tap][c] (dW, A = dY with sam = 1,
 *                 sak = M; B = the layer input [B*121][cs]); N = 9 cs, K = B*121.
 * Out-of-map taps read 0. */
#define EVX_CONV_FWD 1
#define EVX_CONV_DX 2
#define EVX_CONV_DW 3
int evx_conv3x3_gemm(const evx_gemm_desc *g, int32_t mode, int32_t cs, void *stream);
/* Workspace floats (evx_gemm_desc.ws / ws_elems) an evx_conv3x3_gemm call can use: the LDS-staged
   forward (bias / ReLU epilogue) and dX (ReLU gate) kernels over cfg4's layer shapes pack the
   weights there as bf16 hi / lo MFMA fragments; otherwise the split-K partials of
   evx_gemm_ws_elems. Without it the call runs the generic implicit-GEMM kernel. */
int64_t evx_conv3x3_ws_elems(const evx_gemm_desc *g, int32_t mode, int32_t cs);

/* The kernel a descriptor runs on (evx_gemm_plan.route): one constant per kernel or template
 * instantiation the launcher can pick. The choice depends on the precision, the strides, the
 * sizes' divisibility by 4 / 8, the operands' 16-byte alignment, K >= 256 and the workspace. */
#define EVX_ROUTE_NONE 0              /* M, N or K <= 0: nothing is launched */
#define EVX_ROUTE_GEMM128_F32 1       /* gemm128_kernel<float>: exact f32 */
#define EVX_ROUTE_GEMM128_BF16 2      /* gemm128_kernel<__bf16> */
#define EVX_ROUTE_X3_VEC_AB 3         /* gemm128x3_kernel, A and B staged from 16-B loads along k */
#define EVX_ROUTE_X3_VEC_A 4          /* gemm128x3_kernel, A only from 16-B loads */
#define EVX_ROUTE_X3_VEC_B 5          /* gemm128x3_kernel, B only from 16-B loads */
#define EVX_ROUTE_X3_SCALAR 6         /* gemm128x3_kernel, one element per load */
#define EVX_ROUTE_X3_SPLIT_AB 7       /* gemm128x3_kernel on pre-split planes (EVX_GEMM_SPLIT_AB) */
#define EVX_ROUTE_TN3_KMAJOR 8        /* tn3_kernel: A[k][m], B[k][n] */
#define EVX_ROUTE_TN3_AK 9            /* tn3_kernel: A[m][k] k-contiguous, B[k][n] */
#define EVX_ROUTE_TN3_CONV_DW 10      /* tn3_kernel gathering the conv input (EVX_CONV_DW) */
#define EVX_ROUTE_X3_CONV_FWD 11      /* gemm128x3_kernel gathering the taps: forward */
#define EVX_ROUTE_X3_CONV_DX 12       /* gemm128x3_kernel gathering the taps: dX */
#define EVX_ROUTE_X3_CONV_DW 13       /* gemm128x3_kernel gathering the taps: dW */
#define EVX_ROUTE_CONV_LDS16_FWD 14   /* conv3x3_x3_kernel<16, 1>: <= 16 -> 32 channels */
#define EVX_ROUTE_CONV_WREG32_FWD 15  /* conv3x3_wreg_kernel<32, ...>: 32 -> 64 channels */
#define EVX_ROUTE_CONV_LDS64_FWD 16   /* conv3x3_x3_kernel<64, 4>: 64 -> 128 channels */
#define EVX_ROUTE_CONV_LDS64_DX 17    /* conv3x3_x3_kernel<64, 1, dX>: dY 64 -> dX 32 channels */
#define EVX_ROUTE_CONV_LDS128_DX 18   /* conv3x3_x3_kernel<128, 2, dX>: dY 128 -> dX 64 channels */
#define EVX_REDUCE_NONE 0
#define EVX_REDUCE_GENERIC 1          /* splitk_reduce_kernel */
#define EVX_REDUCE_QUARTERS 2         /* splitk_reduce4_kernel: >= 8 slices, M*N a multiple of 4 */
typedef struct {
    int32_t route;   /* EVX_ROUTE_* */
    int32_t slices;  /* K slices (gridDim.z); 1: one pass */
    int32_t klen;    /* K rows per slice (a multiple of 32) */
    int32_t reduce;  /* EVX_REDUCE_* */
} evx_gemm_plan;
/* What evx_gemm (mode 0) or evx_conv3x3_gemm(mode = EVX_CONV_*, cs) would launch for g: decided on
 * the host by the function the launcher itself switches on -- no launch, no device call (the
 * pointers are only tested for NULL and alignment). An argument error the call would report before
 * launching comes back as the same negative code with the same evx_q_last_error text. */
int evx_gemm_plan_query(const evx_gemm_desc *g, int32_t mode, int32_t cs, evx_gemm_plan *out);
/* out[n] (+)= sum_m X[m*ld+n] (bias gradients), fixed summation order. scratch: one partial per
 * 64 rows and column, ceil(M / 64) * N floats; a shorter one (scratch_elems >= N) makes the chunks
 * longer. M <= 0 or N <= 0: 0, nothing done. -22: scratch_elems < N; a NULL X, out or scratch. */
int evx_colsum(const float *X, int64_t ld, int32_t M, int32_t N, float *out, int32_t accum, float *scratch,
               int32_t scratch_elems, void *stream);
/* DQNAgent.learn TD step (agents/dqn_agent.py:143-151): loss = mean((Q[a] - (r + gamma*max Qt * !done))^2),
 * dQ = d loss / d Q. Q, Qt: [B][A]. ws: caller workspace of evx_td_loss_ws_floats(B, nets) floats
 * (the per-block partials of the loss, summed in block order by a second launch: deterministic,
 * no state in the library; calls on different streams need different workspaces). */
int64_t evx_td_loss_ws_floats(int32_t B, int32_t nets);
int evx_td_loss(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                const uint8_t *done, float gamma, int32_t B, float *dQ, float *loss, float *ws, int64_t ws_floats,
                void *stream);
/* evx_td_loss with optional importance weights w [B] (prioritized replay: loss = mean(w (q - y)^2),
 * dQ scaled by w) and optional td_abs [B] = |q - y| (the new priorities); w = td_abs = NULL is
 * evx_td_loss. */
int evx_td_loss_w(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                  const uint8_t *done, float gamma, int32_t B, const float *w, float *dQ, float *loss,
                  float *td_abs, float *ws, int64_t ws_floats, void *stream);
/* evx_td_loss_w plus clearing zero[0..nzero) (the gradient buffer the backward accumulates into)
 * in the same launch (extra workgroups) */
int evx_td_loss_zero(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                     const uint8_t *done, float gamma, int32_t B, const float *w, float *dQ, float *loss, float *td_abs,
                     float *zero, int64_t nzero, float *ws, int64_t ws_floats, void *stream);
/* ||g||_2 into norm[0] (clip_grad_norm_'s total norm). scratch: one partial per 4096 elements, at
 * most min(scratch_elems, 2048) of them. n <= 0 writes norm[0] = 0 (g is not read). -22:
 * scratch_elems < 1; a NULL scratch or norm; a NULL g with n > 0. */
int evx_sumsq_norm(const float *g, int64_t n, float *scratch, int32_t scratch_elems, float *norm, void *stream);
/* g *= min(1, max_norm/(norm+1e-6)) (skipped if norm NULL or max_norm <= 0) then one
 * torch.optim.Adam step (g + weight_decay p when weight_decay != 0; g is written back as used).
 * -22, whatever n: a NULL h; h->step < 1 (the bias corrections divide by 1 - beta^step: step 0
 * would write infinities into every parameter); a beta outside [0, 1) or NaN; a non-finite lr or
 * eps. Then n <= 0: 0, nothing done. -22: a NULL p, g, m or v. */
int evx_clip_adam(float *p, float *g, float *m, float *v, int64_t n, const float *norm, float max_norm,
                  const evx_adam *h, void *stream);
/* nn.Dropout keep-mask (1 with probability 1-p), counter-based Philox4x32-10: element i is lane
 * i % 4 of counter (i / 4 + offset, 0x5eed, 0) under the key seed, kept where u01 >= p; a call uses
 * ceil(n / 4) counters (oracle/draw_oracle.c orc_dropout_mask restates it). -22, whatever n: p
 * outside [0, 1] or NaN. Then n <= 0: 0. -22: a NULL mask. */
int evx_dropout_mask(uint8_t *mask, int64_t n, float p, uint64_t seed, uint64_t offset, void *stream);
/* DQNAgent.act (agents/dqn_agent.py:101-124): epsilon-greedy over argmax_a Q[i][a] */
int evx_act(const float *Q, int32_t n, int32_t A, float epsilon, uint64_t seed, uint64_t offset,
            int32_t *actions, void *stream);
/* DQNAgent.remember for n rows (agents/dqn_agent.py:97-99): row i goes to ring slot
 * (pos + i) mod capacity with a[i], s[i], s2[i] and the team reward (f64 -> f32, round to nearest
 * even) and done flag of env i / agents_per_env. The caller keeps pos and size: pos advances by n
 * mod capacity, size grows to at most capacity.
 * -22 before any launch (evx_q_last_error names the entry): a NULL rp or capacity < 1; a NULL ring
 * array; n < 0; n > capacity (two rows of one push would share a slot, the winner undefined); pos
 * outside [0, capacity); agents_per_env < 1; n no multiple of agents_per_env. Then n == 0: 0,
 * nothing done (s .. done_env may be NULL). -22: a NULL s, s2, a, r_env or done_env. */
int evx_replay_push(const evx_replay *rp, const evx_obs *s, const evx_obs *s2, const int32_t *a,
                    const double *r_env, const uint8_t *done_env, int32_t n, int32_t agents_per_env, int64_t pos,
                    void *stream);
/* evx_replay_push with s2 = done_env[e] ? s2_term : s2 (the terminal observations of
 * envs that evx_env_step auto-reset); s2_term may be NULL (evx_replay_push). The same refusals. */
int evx_replay_push_term(const evx_replay *rp, const evx_obs *s, const evx_obs *s2, const evx_obs *s2_term,
                         const int32_t *a, const double *r_env, const uint8_t *done_env, int32_t n,
                         int32_t agents_per_env, int64_t pos, void *stream);
/* evx_replay_push_term and evx_env_orders (the next step's order and the next act's env order
 * `perm`, from the class bytes of state `s`) in one launch; the replay capacity must be a power of
 * two. Replaces DQNAgent.remember for every robot of a step (agents/dqn_agent.py:97-99) plus the
 * scheduling permutations. */
int evx_env_orders_push(const evx_layout *l, const evx_state *s, int32_t *perm, const evx_replay *rp,
                        const evx_obs *s_obs, const evx_obs *s2, const evx_obs *s2_term, const int32_t *a,
                        const double *r_env, const uint8_t *done_env, int32_t n, int32_t agents_per_env,
                        int64_t pos, void *stream);
/* ... and the learn step's batch (evx_replay_sample over the ring as it stands after the push:
 * size = the ring size after it; B = 0 draws nothing) in the same launch; a drawn slot inside the
 * push window is read from the push's sources.
 * -22 before any launch, whether or not B > 0: a bad layout or state; a capacity that is no power
 * of two; and what evx_replay_push_term refuses (a NULL ring array, n < 0, n > capacity, pos outside
 * [0, capacity), agents_per_env < 1, n no multiple of it, a NULL source array with n > 0). With
 * B > 0 also: size outside [1, capacity], B > size, a NULL output. */
int evx_env_orders_push_sample(const evx_layout *l, const evx_state *s, int32_t *perm, const evx_replay *rp,
                               const evx_obs *s_obs, const evx_obs *s2, const evx_obs *s2_term, const int32_t *a,
                               const double *r_env, const uint8_t *done_env, int32_t n, int32_t agents_per_env,
                               int64_t pos, int32_t B, int64_t size, uint64_t seed, uint64_t offset, evx_obs *out_s,
                               evx_obs *out_s2, int32_t *out_a, float *out_r, uint8_t *out_done, void *stream);
/* random.sample replacement for the vectorised learner (agents/dqn_agent.py:132): row i of the
 * outputs is the ring's row at slot perm(i), for a keyed pseudo-random permutation perm of
 * [0, size) (a 6-round Feistel network, cycle-walked; the key is all 128 bits of (seed, offset));
 * idx_out (may be NULL) gets the slots. Without replacement: B = size draws visit every slot once.
 * Documented limit: the first draw is uniform and the joint distribution of the draws close to
 * uniform only from a few dozen entries on -- below 32 entries the pairs of draws are measurably
 * non-uniform, and at some sizes below 15 a slot's frequency as first draw is off 1/size by up to
 * 3 % (DESIGN.md section 5.0 has the measurements). Trainers sample rings no smaller than a batch.
 * -22 before any launch: a NULL rp or size < 1. Then B <= 0: 0, nothing done (the outputs may be
 * NULL). -22: size > capacity; B > size (as random.sample raises); a NULL ring array; a NULL s, s2,
 * a, r or done. */
int evx_replay_sample(const evx_replay *rp, int64_t size, int32_t B, uint64_t seed, uint64_t offset, evx_obs *s,
                      evx_obs *s2, int32_t *a, float *r, uint8_t *done, int64_t *idx_out, void *stream);
/* B uniform indices over the ring window [base, base+count) mod capacity (same draws as
 * evx_replay_sample with base 0): lets a learn step sample the transitions already pushed
 * while the next push overwrites the slots outside the window (lagged-replay schedule).
 * -22 before any launch: a NULL rp or count < 1; count > capacity or base outside [0, capacity).
 * Then B <= 0: 0. -22: B > count; a NULL ring array; a NULL s, s2, a, r or done. */
int evx_replay_sample_window(const evx_replay *rp, int64_t base, int64_t count, int32_t B, uint64_t seed,
                             uint64_t offset, evx_obs *s, evx_obs *s2, int32_t *a, float *r, uint8_t *done,
                             int64_t *idx_out, void *stream);
/* One memory per agent (runners/train_double_dqn.py:50-51: agent_i.remember / learn on its own
 * transitions): with pushes of whole envs (rows env * nets + agent, capacity % nets == 0) the
 * agent's transitions are the ring slots == agent (mod nets); B uniform draws among them
 * (among the first size slots) for every agent, into rows [agent B, (agent + 1) B). */
int evx_replay_sample_agents(const evx_replay *rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                             uint64_t offset, evx_obs *s, evx_obs *s2, int32_t *a, float *r, uint8_t *done,
                             void *stream);
/* The joint memory of runners/train_qmix.py:36,78-96 (one entry per env-step, all agents'
 * observations and actions): draw i picks the same env-step for every agent (rows agent B + i
 * hold that agent's slot); counters offset + i. */
int evx_replay_sample_joint(const evx_replay *rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                            uint64_t offset, evx_obs *s, evx_obs *s2, int32_t *a, float *r, uint8_t *done,
                            void *stream);
/* n-step rows of sampled slots (no counterpart in the reference, whose target is one step deep).
 * Every training step pushes `stride` rows in the same order (env * R + robot), so the successor
 * of slot j -- same env, same robot, next env step -- is slot (j + stride) mod capacity while that
 * slot is inside the live range [base, base + count) mod capacity (push order, oldest first: the
 * whole ring is ((pos - size) mod capacity, size), the lagged schedule's window is the pair given
 * to evx_replay_sample_window). idx [B]: the samplers' idx_out. Per row, all f32, a multiply and
 * an add (no fma):
 *   j0 = idx[i];  d0 = (j0 - base) mod C;  j = j0;  R = r[j0];  g = gamma;  dn = done[j0];  L = 1
 *   while L < n_step and !dn and d0 + L stride < count:
 *       j = (j0 + L stride) mod C;  R = R + g r[j];  g = g gamma;  dn = done[j];  L = L + 1
 *   r[i] = R;  gamma_row[i] = g;  done[i] = dn;  s2[i] = rp.s2[j];  len[i] = L   (len may be NULL)
 * so y = R + gamma_row * Q_target(s2, .) * !done (evx_td_opts.gamma_row). The chain stops at a
 * terminal slot (never across an auto-reset) and at the end of the range; a row with d0 >= count
 * keeps its own slot (L = 1); n_step = 1 copies the slot's r, done, s2 and gamma_row = gamma.
 * -22 before any launch: a NULL rp, idx, s2, r, done or gamma_row (len may be NULL), n_step outside
 * [1, EVX_NSTEP_MAX], stride < 1, count outside [0, capacity], base outside [0, capacity), gamma
 * not finite (evx_q_last_error). Then B <= 0: 0. -22: a ring without its s2, r or done array. */
#define EVX_NSTEP_MAX 32
int evx_replay_nstep(const evx_replay *rp, const int64_t *idx, int32_t B, int64_t base, int64_t count,
                     int64_t stride, int32_t n_step, float gamma, evx_obs *s2, float *r, uint8_t *done,
                     float *gamma_row, int32_t *len, void *stream);
/* evx_replay_sample_agents (joint = 0) or evx_replay_sample_joint (joint != 0) and evx_replay_nstep
 * in one launch, for per-robot and QMIX nets. Row g B + i draws slot j0 as that sampler does with
 * the same (size, B, nets, seed, offset), takes s and a from it and follows evx_replay_nstep's chain
 * from j0 over the live range [base, base + count) mod capacity (successor of slot j: (j + stride)
 * mod capacity; stride = the rows of one push, a multiple of nets, so a chain stays with its agent;
 * it stops at n_step, at a terminal slot or at the end of the range): r = the discounted return,
 * s2 / done = the chain's last slot's, gamma_row = gamma^L, len = L (int32 [nets][B], may be NULL),
 * idx_out = j0 (int64 [nets][B], may be NULL). All f32, R + g r a multiply and an add. n_step = 1:
 * the sampler's s / s2 / a / r / done bit for bit, gamma_row = gamma, len = 1. A stride beyond the
 * ring is taken as the capacity.
 * Joint mode: the push writes the env's team reward and done flag into every robot's row, so the
 * nets chains of one draw have the same length, return and done flag: agent 0's r / done /
 * gamma_row, rows [0, B), are the joint row's (what evx_qmix_loss_opt takes).
 * -22 before any launch: a NULL rp, s, s2, a, r, done or gamma_row, a capacity < 1, n_step outside
 * [1, EVX_NSTEP_MAX], stride < 1, count outside [0, capacity], base outside [0, capacity), gamma not
 * finite (evx_q_last_error). Then B <= 0: 0. -22: nets outside 1..65535, a capacity or size that is
 * no multiple of nets, size outside [nets, capacity], B > size / nets, a NULL ring array. */
int evx_replay_sample_nstep_agents(const evx_replay *rp, int64_t size, int32_t B, int32_t nets, int32_t joint,
                                   uint64_t seed, uint64_t offset, int64_t base, int64_t count, int64_t stride,
                                   int32_t n_step, float gamma, evx_obs *s, evx_obs *s2, int32_t *a, float *r,
                                   uint8_t *done, float *gamma_row, int32_t *len, int64_t *idx_out, void *stream);
/* ------------------------------------------- prioritized replay
 * Proportional prioritized replay (Schaul et al. 2016) over the slots of an evx_replay
 * ring; the reference samples uniformly (random.sample, agents/dqn_agent.py:132), so
 * this is the build's own extension, pinned by oracle/prio_oracle.c. Two segment trees
 * in heap layout over capacity C = 2^k slots (node n = child 2n (op) child 2n+1, root 1,
 * slot i at leaf C + i): sums and minima of the leaf priorities p_i^alpha. Empty or
 * hidden slots hold 0 in the sum tree and +inf in the min tree. New transitions get the
 * largest leaf priority set so far (max_leaf, initially 1). */
typedef struct {
    int64_t capacity;   /* power of two, 2^10 <= C <= 2^26 */
    double *sum;        /* [2C] */
    double *mn;         /* [2C] */
    double *max_leaf;   /* [1] */
    int32_t *owner;     /* [C] scratch for evx_prio_update, all -1 (evx_prio_init sets it) */
} evx_prio;

/* all leaves empty (sum 0, min +inf), max_leaf = 1, owner = -1 */
int evx_prio_init(const evx_prio *t, void *stream);
/* Slots [pos, pos + n_new) mod C get priority max_leaf (newly pushed transitions) and
 * slots [pos + n_new, pos + n_new + n_hide) mod C get priority 0 (hidden: about to be
 * overwritten by a push running concurrently -- the lagged schedule); both trees are
 * rebuilt over the touched leaf blocks. n_new + n_hide <= C. */
int evx_prio_set_range(const evx_prio *t, int64_t pos, int64_t n_new, int64_t n_hide, void *stream);
/* Leaf idx[k] = (td_abs[k] + eps)^alpha for k = 0..B-1 (a later k wins over an earlier
 * one with the same slot, as a sequential loop), max_leaf updated, trees rebuilt.
 * A row whose priority is not finite (td_abs NaN or +inf) leaves its slot's leaf and max_leaf
 * as they were. It still takes part in ownership: the last row naming a slot owns it, so a slot
 * whose last row is not finite keeps the leaf it had before the call. The trees therefore stay
 * finite whatever the learner's |TD| holds. owner is all -1 again when the call has run. */
int evx_prio_update(const evx_prio *t, const int64_t *idx, const float *td_abs, int32_t B, double eps,
                    double alpha, void *stream);
/* Stratified proportional sampling: for k = 0..B-1, u = (k + U_k) * (total / B) with U_k a
 * 53-bit uniform from Philox4x32-10(counter offset + k, key seed); descend the sum tree
 * (left if u < sum[left] or sum[right] <= 0, else u -= sum[left] and right). Gathers the
 * transitions like evx_replay_sample and writes the importance weights
 * w_k = (p_k / p_min)^(-beta) (= (N P(k))^-beta / max_j (N P(j))^-beta). */
int evx_prio_sample(const evx_replay *rp, const evx_prio *t, int32_t B, double beta, uint64_t seed,
                    uint64_t offset, evx_obs *s, evx_obs *s2, int32_t *a, float *r, uint8_t *done,
                    int64_t *idx_out, float *w_out, void *stream);

const char *evx_prio_last_error(void);

/* ---- static floor field on the device ------------------------------------
 * Replaces Map.Init_Potential (envs/map.py:127-148) for n_layouts layouts of one padded grid
 * size GX x GY (= (L+2) x (W+2)), one workgroup each, bit-identical to the reference's heapq
 * Dijkstra. Per layout, row-major [GX][GY]:
 *   valid  u8  Map.Check_Valid on the pre-potential grid (1 <= x <= L, 1 <= y <= W, space != inf)
 *   source u8  the exits (Map.Exit: distance 1)
 *   pen    f64 200 * danger(t=0, (i, j)) ** 2 (envs/map.py:143-146; NULL = no fire term)
 *   floor  f64 out: Map.space after Init_Potential (inf where unreachable)
 *   passes i32 [n_layouts] relaxation passes used (may be NULL; diagnostics) */
int evx_floor_field(int32_t n_layouts, int32_t GX, int32_t GY, const uint8_t *valid, const uint8_t *source,
                    const double *pen, double *floor, int32_t *passes, void *stream);
const char *evx_floor_last_error(void);

/* dst[i] = src[idx[i]], i < n (idx within the source: not checked). n <= 0: 0. -22: a NULL src,
 * idx or dst. */
int evx_gather_obs(const evx_obs *src, const int64_t *idx, int32_t n, evx_obs *dst, void *stream);
/* DQNNetwork conv layers (agents/dqn_agent.py:22-24) as im2col + GEMM on 11x11 maps: x [B][C][11][11]
 * (nhwc: [B][11][11][C]) <-> cols [B*121][C*9], k = c*9 + ky*3 + kx; col2im sums the <= 9 taps of an
 * input element in a fixed order. These two, evx_pix_split and evx_pix_nchw: B <= 0: 0, nothing done
 * (whatever C); else -22 for C < 1 and for a NULL pointer. */
int evx_im2col3x3(const float *x, int32_t B, int32_t C, int32_t nhwc, float *cols, void *stream);
int evx_col2im3x3(const float *dcols, int32_t B, int32_t C, float *dx, void *stream);
/* NCHW [B][C][121] f32 -> pixel-major [B][121*C] as bf16 hi / lo planes (lo B*121*C elements after
   hi): the x3 operand of an EVX_GEMM_SPLIT_AB GEMM (the conv net's fc1 weights), C <= 134 */
int evx_pix_split(const float *src, int32_t B, int32_t C, uint16_t *dst, void *stream);
/* [B*121][C] pixel-major <-> [B][C][121] NCHW (to_nchw): through LDS for C <= 134, element-wise
   beyond (any C) */
int evx_pix_nchw(const float *src, int32_t B, int32_t C, int32_t to_nchw, float *dst, void *stream);
/* dy[i] = y[i] > 0 ? dy[i] : 0 (a NaN y zeroes dy). n <= 0: 0. -22: a NULL dy or y. */
int evx_relu_grad(float *dy, const float *y, int64_t n, void *stream);
const char *evx_q_last_error(void);

/* ------------------------------------------------- MLP Q-network fast path (bf16 MFMA)
 * DQNNetwork's fc stack (agents/dqn_agent.py:40-61; MLP variant 726-512-256-5) with the
 * observation expansion of EvacuationEnv._get_state (envs/evacuation_env.py:84-120)
 * generated inside fc1, and DQNAgent.act's epsilon-greedy (:101-124) fused after fc3.
 * Dropout keep bits are a counter hash of (seed, stream, row, col): the backward pass
 * regenerates them. */
typedef struct {
    const uint16_t *w1;   /* [512][512] bf16 fc1.weight over the compact K (evx_qmlp_pack), MFMA operand-tiled */
    const float *b1c;     /* [512] fc1.bias + bf16(fc1.weight[:, 365]) (the constant centre channel), evx_qmlp_pack */
    const uint16_t *w2;   /* [256][512] bf16 fc2.weight, MFMA operand-tiled (evx_qmlp_pack) */
    const uint16_t *w2t;  /* [512][256] bf16 fc2.weight transposed (backward), may be NULL for forward */
    const float *b2;      /* [256] */
    const float *w3;      /* [5][256] f32 fc3.weight */
    const float *b3;      /* [5] */
    /* act fast path (evx_qmlp_act), optional: fc1's occupancy columns [512][128] bf16 (evx_qmlp_pack's
     * w1o) and the pre-activation table of evx_qmlp_stat for observations at fire step stat_fs */
    const uint16_t *w1o;
    const float *stat;
    int32_t stat_fs;
    /* x3 = 1: f32-accurate arithmetic (the reference's fp32 DQNNetwork): every f32 operand v is
     * carried as bf16 hi = bf16(v) plus lo = bf16(v - hi) and a product as hi*hi + hi*lo + lo*hi
     * on the bf16 MFMA (exact 0/1 operands skip their lo); w1 then spans K = 640 (compact K +
     * one danger-residual slot per cell), w1l / w2l / w2tl hold the lo parts (evx_qmlp_pack3) */
    int32_t x3;
    const uint16_t *w1l, *w2l, *w2tl;
    /* x3 act fast path: the lo part of w1o (w1o then holds the hi part; evx_qmlp_pack3 / _adam_pack3) */
    const uint16_t *w1ol;
    /* the table's window centres: x in [stat_x0, stat_x0 + stat_nx) (Map.robot_range: robots never
     * leave it), every y in [0, W + 1], row (x - stat_x0) * (W + 2) + y; stat_nx = 0: all L + 2 */
    int32_t stat_x0, stat_nx;
    /* x3, optional: the table rows' fc1 inputs (evx_qmlp_expand_x3 of the table's observations, the X of
     * evx_qmlp_stat_x): the learner's X of a batch row on the table path is that row of it plus the
     * row's occupancy bits (copied instead of regenerated; the same bits) */
    const uint16_t *stat_xin;
} evx_qmlp_params;

typedef struct {
    uint32_t seed, stream; /* mask identity */
    float p;               /* drop probability; 0 = eval (no dropout) */
    uint32_t row0;         /* hash row of the batch's first row (even): a rank's act masks keyed by the
                            * global agent id, so trajectories do not depend on the GPU count */
    const uint8_t *mask;   /* optional explicit keep mask [n][512] (1 = keep; scale 1/(1-p)) in place of
                            * the hash: replays the reference's captured torch dropout masks */
} evx_qmlp_dropout;

typedef struct {
    uint16_t *h1;          /* [n][512] bf16 fc1 output after ReLU + dropout (required) */
    uint16_t *x;           /* [n][512] bf16 compact expanded observation, or NULL */
    float *h2;             /* [n][256] fc2 output after ReLU, or NULL */
    float *q;              /* [n][5] Q values, or NULL */
    int32_t *actions;      /* [n] epsilon-greedy actions (evx_act's rule and RNG), or NULL */
    float epsilon;
    uint64_t act_seed, act_offset;
    /* x3: h1 holds two planes [2][n][512] (hi, lo) and x spans [n][640] */
    /* act only, optional: batch row i is observation / action row perm[i / rows_per_env] * rows_per_env +
     * i % rows_per_env (evx_act_perm: envs at the table's fire step first, so act tiles are uniform);
     * dropout rows and epsilon draws stay keyed by that original row; rows_per_env even (dropout
     * row pairs stay together) */
    const int32_t *perm;
    int32_t rows_per_env;
    /* act only, optional: int32 workspace of evx_qmlp_act_ws_ints(n) elements, zeroed once by the
     * caller (every act leaves its two counters zeroed; one workspace per act in flight). With it the x3 persistent act lists
     * the 128-row tiles it leaves to the 64-row kernel (a row below stat_fs or a centre outside the
     * table), so that kernel runs only those instead of re-checking every row (NULL: it re-checks). */
    int32_t *act_ws;
} evx_qmlp_fwd_out;

/* elements of evx_qmlp_fwd_out.act_ws for an act of n rows */
int64_t evx_qmlp_act_ws_ints(int32_t n);

/* bf16 copies of fc1.weight [512][726] over fc1's compact K and fc2.weight [256][512]
 * (w2t may be NULL), and b1c. Compact K: 4 features per cell c < 121 at k = 4c + f for
 * the reference's channels f + 1 (occupancy, danger, barrier, exit), k >= 484 zero; the
 * reference's channel 0 is identically zero and channel 5 is the constant centre
 * one-hot, folded into b1c. */
int evx_qmlp_pack(const float *w1, const float *b1, const float *w2, uint16_t *w1b, float *b1c, uint16_t *w2b,
                  uint16_t *w2t, uint16_t *w1o, void *stream);
/* x3 (f32-accurate) operand copies: w1b [512][640] hi (compact K, then the danger column of cell
 * c at k = 512 + c, multiplying the danger residual), w1l [512][512] lo of the compact K, w2b / w2l
 * hi / lo of fc2.weight, w2t / w2tl of its transpose (may be NULL); b1c = b1 + W1[:, centre] in f32 */
int evx_qmlp_pack3(const float *w1, const float *b1, const float *w2, uint16_t *w1b, uint16_t *w1l, float *b1c,
                   uint16_t *w2b, uint16_t *w2l, uint16_t *w2t, uint16_t *w2tl, void *stream);
/* x3 act fast path operands: fc1's occupancy columns [512][128] as hi (w1o) and lo (w1ol) bf16, w1o_tile order */
int evx_qmlp_pack_occ3(const float *w1, uint16_t *w1o, uint16_t *w1ol, void *stream);
/* fc1's pre-activation (X W1^T + b1, f32, no ReLU / dropout) of n observations -> out [n][512]:
 * with obs = every window centre of the layout at one fire step and zero occupancy this is the
 * act fast path's table (evx_qmlp_params.stat; rebuild after every weight update) */
int evx_qmlp_stat(const evx_layout *lay, const evx_obs *obs, int32_t n, const evx_qmlp_params *p, float *out,
                  void *stream);
/* x3: the rows' compact fc1 inputs [n][640] bf16 (4 features per cell, then the cells' danger
 * residuals: the X of evx_qmlp_fwd_out.x) of n observations */
int evx_qmlp_expand_x3(const evx_layout *lay, const evx_obs *obs, int32_t n, uint16_t *x, void *stream);
/* evx_qmlp_stat (x3) from the rows' X of evx_qmlp_expand_x3 instead of their observations: the same
 * table bit for bit, with fc1's A operand read instead of generated (the act table's rows are fixed,
 * so their X is expanded once; x NULL: evx_qmlp_stat) */
int evx_qmlp_stat_x(const evx_layout *lay, const evx_obs *obs, const uint16_t *x, int32_t n, const evx_qmlp_params *p,
                    float *out, void *stream);
int evx_qmlp_forward(const evx_layout *lay, const evx_obs *obs, int32_t n, const evx_qmlp_params *p,
                     const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out, void *stream);
/* DQNAgent.act (agents/dqn_agent.py:101-124) in one launch: the forward of
 * evx_qmlp_forward with H1 and H2 kept on chip (out->h1, x, h2 ignored), writing
 * out->q and/or out->actions; bit-identical to evx_qmlp_forward's, except that 128-row tiles
 * whose observations are all at p->stat_fs start fc1 from p->stat (when p->w1o / p->stat are
 * set): the same products summed in another order. */
int evx_qmlp_act(const evx_layout *lay, const evx_obs *obs, int32_t n, const evx_qmlp_params *p,
                 const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out, void *stream);
/* The same act on the 64-row kernel only. x3 evx_qmlp_act runs a persistent kernel of 128-row tiles
 * (one workgroup per CU) when the table path is attached, the dropout is the hash or off and n
 * covers 4 tiles per CU; it gives the same bits as this one (tests compare the two). */
int evx_qmlp_act64(const evx_layout *lay, const evx_obs *obs, int32_t n, const evx_qmlp_params *p,
                   const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out, void *stream);
/* Two forwards of n rows in one launch pair (the learner's online and target nets). */
int evx_qmlp_forward2(const evx_layout *lay, int32_t n, const evx_obs *obs0, const evx_qmlp_params *p0,
                      const evx_qmlp_dropout *drop0, const evx_qmlp_fwd_out *out0, const evx_obs *obs1,
                      const evx_qmlp_params *p1, const evx_qmlp_dropout *drop1, const evx_qmlp_fwd_out *out1,
                      void *stream);

/* fp32 gradient tensors (the reference's parameter shapes: fc1.weight [512][726], ...) */
typedef struct {
    float *w1, *b1, *w2, *b2, *w3, *b3;
    /* required scratch of the backward's partial sums, evx_qmlp_backward_part_floats(B) floats
     * (weight-gradient split-K tiles, fc3 / bias block rows): every gradient sum is added in a
     * fixed order -- the same bits on every run, no f32 atomics */
    float *part;
} evx_qmlp_grads;
int64_t evx_qmlp_backward_part_floats(int32_t B);

/* loss.backward() of DQNAgent.learn (agents/dqn_agent.py:150-158) for the saved online
 * forward (x, h1, h2 of evx_qmlp_forward) given dQ = d loss / d Q [B][5]. zero_grads != 0: the
 * gradients are overwritten (every element), else added to. dz2 [B][256] and dz1
 * [B][512] are bf16 scratch. Needs p->w2t. With p->x3 the activations are the x3 forward's
 * (h1 two planes, x 640 wide), dz2 / dz1 hold two planes each (hi, lo) and every product
 * is split as in the forward. */
int evx_qmlp_backward(const evx_qmlp_params *p, int32_t B, const float *dq, const uint16_t *x, const uint16_t *h1,
                      const float *h2, float drop_p, uint16_t *dz2, uint16_t *dz1, const evx_qmlp_grads *g,
                      int32_t zero_grads, void *stream);
/* evx_qmlp_backward that also leaves clip_grad_norm_'s squared-norm partials of the final gradients
 * in ss[0 .. evx_qmlp_norm_parts()) (the gradients one flat state_dict-order buffer: g->w1 .. g->b3
 * contiguous); with g->part the weight-gradient reductions and the partials share one launch. */
int evx_qmlp_backward_ss(const evx_qmlp_params *p, int32_t B, const float *dq, const uint16_t *x, const uint16_t *h1,
                         const float *h2, float drop_p, uint16_t *dz2, uint16_t *dz1, const evx_qmlp_grads *g,
                         int32_t zero_grads, float *ss, void *stream);
/* DQNAgent.learn's TD step and loss.backward() in one (agents/dqn_agent.py:143-158): dQ from the
 * online Q [B][5], the target Qt [B][5], actions, rewards, done flags and gamma (as evx_td_loss_w,
 * importance weights w or NULL) inside the backward's first kernel; loss[0] = the mean (weighted)
 * squared TD error, td_abs [B] = |TD error| (or NULL); the gradients overwritten; ss as in
 * evx_qmlp_backward_ss, or NULL (no norm partials: an all-reduce will change the gradients). */
int evx_qmlp_td_backward_ss(const evx_qmlp_params *p, int32_t B, const float *Q, const float *Qt, const int32_t *act,
                            const float *rew, const uint8_t *done, float gamma, const float *w, float *loss,
                            float *td_abs, const uint16_t *x, const uint16_t *h1, const float *h2, float drop_p,
                            uint16_t *dz2, uint16_t *dz1, const evx_qmlp_grads *g, float *ss, void *stream);
int32_t evx_qmlp_norm_parts(void);
int64_t evx_qmlp_nparams(void);
/* the same partials of a flat gradient buffer (after an all-reduce changed it) */
int evx_qmlp_sumsq_parts(const float *g, float *ss, void *stream);
/* clip_grad_norm_ + Adam (agents/dqn_agent.py:158-160) on the MLP's flat p / g / m / v (state_dict
 * order, evx_qmlp_nparams() elements) from the nss norm partials, with the x3 operand repack
 * (evx_qmlp_pack3's outputs) in the same launch; g receives the clipped gradients, norm_out (or
 * NULL) the total norm. Replaces evx_sumsq_norm + evx_clip_adam + evx_qmlp_pack3. */
int evx_qmlp_adam_pack3(float *p, float *g, float *m, float *v, float max_norm, const evx_adam *h, uint16_t *w1b,
                        uint16_t *w1l, float *b1c, uint16_t *w2b, uint16_t *w2l, uint16_t *w2t, uint16_t *w2tl,
                        uint16_t *w1o, uint16_t *w1ol, const float *ss, int32_t nss, float *norm_out, void *stream);
const char *evx_qmlp_last_error(void);

/* ---- Grouped independent nets: runners/train_double_dqn.py:35-56 trains one
 * DQNAgent per robot, runners/train_qmix.py:78-118 one per agent under a mixer. `nets` MLPs in
 * one launch per kernel: every per-net buffer is an array [nets][one net's buffer] and the
 * pointers passed are net 0's (x3 parameters: evx_qmlp_pack3 layout per net; flat parameters,
 * gradients, m, v [nets][evx_qmlp_nparams()]). */
/* DQNAgent.act of net g for rows i*nets + g of obs / q / actions (robot g of env i uses net g),
 * n rows per net (even); dropout rows keyed g*n + i, epsilon draws by the data row. No
 * permutation, no table path (p->stat NULL). */
int evx_qmlp_act_g(const evx_layout *lay, const evx_obs *obs, int32_t n, int32_t nets, const evx_qmlp_params *p,
                   const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out, void *stream);
/* evx_qmlp_forward2 for nets blocked problems: net g reads obs rows [g n, (g + 1) n) and writes
 * its [n]-row blocks of h1 (two planes) / x / h2 / q; dropout rows keyed g*n + row. */
int evx_qmlp_forward2_g(const evx_layout *lay, int32_t n, int32_t nets, const evx_obs *obs0,
                        const evx_qmlp_params *p0, const evx_qmlp_dropout *drop0, const evx_qmlp_fwd_out *out0,
                        const evx_obs *obs1, const evx_qmlp_params *p1, const evx_qmlp_dropout *drop1,
                        const evx_qmlp_fwd_out *out1, void *stream);
/* evx_td_loss_zero per net: rows [g B, (g + 1) B) of Q / Qt / act / rew / done / dQ, loss[g]
 * = mean over the net's rows; ws of evx_td_loss_ws_floats(B, nets) floats. */
int evx_td_loss_zero_g(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                       const uint8_t *done, float gamma, int32_t B, int32_t nets, const float *w, float *dQ,
                       float *loss, float *td_abs, float *zero, int64_t nzero, float *ws, int64_t ws_floats,
                       void *stream);

/* ---- TD options: Double-Q targets, Huber loss, soft target updates. None of them has a
 * counterpart in the reference (agents/dqn_agent.py:143-151 is the max target with the MSE and
 * a hard copy); all off gives the entries above bit for bit. Per row, all f32:
 *   j* = sel ? clamp(sel[i], 0, A - 1) : argmax_j Qt[i][j]
 *   y  = rew[i] + (gamma * Qt[i][j*]) * (done[i] ? 0 : 1);  d = Q[i][act[i]] - y;  td_abs[i] = |d|
 *        (gamma_row given: gamma_row[i] in place of gamma)
 *   huber_delta = 0:  l = d * d,  g = 2 d
 *   huber_delta > 0:  l = |d| <= delta ? 0.5 (d * d) : delta (|d| - 0.5 delta),  g = min(max(d, -delta), delta)
 *   (l and g times w[i] with weights);  dQ[i][act[i]] = g / B;  loss = mean(l). */
typedef struct {
    const int32_t *sel;   /* [B] (grouped: [nets][B]) action whose target value bootstraps:
                             y uses Qt[i][sel[i]]; NULL: max_j Qt[i][j] */
    float huber_delta;    /* 0: squared error; > 0: Huber loss with this delta */
    const float *gamma_row; /* [B] (grouped: [nets][B]) the row's discount in place of gamma in y
                               (n-step rows: evx_replay_nstep's gamma^L); NULL: the scalar gamma */
} evx_td_opts;
/* evx_td_loss_zero_g with options (nets = 1: evx_td_loss_zero; zero = NULL: evx_td_loss_w);
 * opt = NULL: no options */
int evx_td_loss_opt(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                    const uint8_t *done, float gamma, int32_t B, int32_t nets, const float *w, float *dQ,
                    float *loss, float *td_abs, float *zero, int64_t nzero, float *ws, int64_t ws_floats,
                    const evx_td_opts *opt, void *stream);
/* evx_qmlp_td_backward_ss with options (opt = NULL: none) */
int evx_qmlp_td_backward_opt(const evx_qmlp_params *p, int32_t B, const float *Q, const float *Qt, const int32_t *act,
                             const float *rew, const uint8_t *done, float gamma, const float *w, float *loss,
                             float *td_abs, const uint16_t *x, const uint16_t *h1, const float *h2, float drop_p,
                             uint16_t *dz2, uint16_t *dz1, const evx_qmlp_grads *g, float *ss,
                             const evx_td_opts *opt, void *stream);
/* Polyak target update: t = tau * p + one_minus_tau * t, elementwise over n floats; tau in [0, 1],
 * one_minus_tau = (float)(1.0 - (double)tau) from the caller */
int evx_polyak(const float *p, float *t, int64_t n, float tau, float one_minus_tau, void *stream);
/* the same blend on the MLP's flat target parameters t (evx_qmlp_nparams() floats) with the
 * target's x3 operand repack (evx_qmlp_pack3's outputs; w1o / w1ol: evx_qmlp_pack_occ3's, or both
 * NULL) in the same launch, as evx_qmlp_adam_pack3 does for the online net */
int evx_qmlp_polyak_pack3(const float *p, float *t, float tau, float one_minus_tau, uint16_t *w1b, uint16_t *w1l,
                          float *b1c, uint16_t *w2b, uint16_t *w2l, uint16_t *w2t, uint16_t *w2tl,
                          uint16_t *w1o, uint16_t *w1ol, void *stream);

/* evx_qmlp_backward_ss for the blocked forward of evx_qmlp_forward2_g (gradients cleared by the
 * caller); g->part: [nets][evx_qmlp_backward_part_floats(B)], ss [nets][evx_qmlp_norm_parts()]. */
int evx_qmlp_backward_ss_g(const evx_qmlp_params *p, int32_t B, int32_t nets, const float *dq, const uint16_t *x,
                           const uint16_t *h1, const float *h2, float drop_p, uint16_t *dz2, uint16_t *dz1,
                           const evx_qmlp_grads *g, float *ss, void *stream);
/* evx_qmlp_adam_pack3 per net (clip_grad_norm_ per agent, train_qmix.py:107-109); ss
 * [nets][nss], norm_out [nets] or NULL. */
int evx_qmlp_adam_pack3_g(float *p, float *g, float *m, float *v, float max_norm, const evx_adam *h, uint16_t *w1b,
                          uint16_t *w1l, float *b1c, uint16_t *w2b, uint16_t *w2l, uint16_t *w2t, uint16_t *w2tl,
                          uint16_t *w1o, uint16_t *w1ol, const float *ss, int32_t nss, float *norm_out, int32_t nets,
                          void *stream);
/* evx_qmlp_adam_pack3_g with a learning rate per net: lr [nets] on the host, net g's step size
 * (float)(lr[g] / (1 - beta1^step)) -- the expression of h->lr in the entries above, so equal lr give
 * evx_qmlp_adam_pack3_g bit for bit; h->lr is not read. Betas, eps, step, weight decay and max_norm are
 * common to the nets. -22 before any launch: a NULL required pointer, nets outside 1..64, an lr that
 * is not finite. */
int evx_qmlp_adam_pack3_gl(float *p, float *g, float *m, float *v, float max_norm, const evx_adam *h, uint16_t *w1b,
                           uint16_t *w1l, float *b1c, uint16_t *w2b, uint16_t *w2l, uint16_t *w2t, uint16_t *w2tl,
                           uint16_t *w1o, uint16_t *w1ol, const float *ss, int32_t nss, float *norm_out, int32_t nets,
                           const float *lr, void *stream);
/* The launch shape of the grouped x3 learn chain (evx_qmlp_forward2_g, evx_td_loss_zero_g,
 * evx_qmlp_backward_ss_g) at B rows per net: every figure depends on B and nets alone. */
typedef struct {
    int32_t fc1_rows;    /* rows per qfc1 tile of the forward pair: 64 (qfc1_kernel<2, 1, 4>) or 128
                            (qfc1_kernel<4, 1, 8>, from 384 tiles x problems x nets) */
    int32_t qbwd3_rows;  /* rows per qbwd3 block: 32, 16, 64 or 128 */
    int32_t dw1_kper;    /* rows per K split of dW1 = dZ1^T X (a multiple of 64) */
    int32_t dw1_gz;      /* its splits per net = ceil(B / dw1_kper): the last may be short */
    int32_t dw2_kper;    /* the same of dW2 = dZ2^T H1 */
    int32_t dw2_gz;
    int32_t qdz1_tiles;  /* 64-row dZ1 tiles per workgroup */
    int32_t td_blocks;   /* 256-row TD-loss blocks (partials) per net */
} evx_qmlp_plan;
/* Decided on the host by the function the chain's launchers themselves call: no launch, no device
 * call. nets = 1 describes the backward only: its figures are those of the single-net x3 backward
 * (evx_qmlp_backward_ss, evx_qmlp_td_backward_ss), while fc1_rows is evx_qmlp_forward2_g's with one
 * net -- what evx_qmlp_forward2 runs is evx_qmlp_fwd_plan_query's to say.
 * -22 for nets outside 1..1024, B <= 0 or out = NULL. */
int evx_qmlp_group_plan(int32_t B, int32_t nets, evx_qmlp_plan *out);

/* What a forward or act entry point launches (evx_qmlp_fwd_plan.route). */
#define EVX_FWD_NONE 0              /* n <= 0: nothing is launched */
#define EVX_FWD_FC 1                /* qfc1_kernel, then qfc23_kernel if fc23_rows: one problem or two
                                       (evx_qmlp_stat, _stat_x: fc1 alone, writing the table) */
#define EVX_FWD_FC_GROUPED 2        /* the same on the grouped instantiations (blockIdx.z = net x problem) */
#define EVX_FWD_PAIRED 3            /* x_expand_kernel + qfwd2_kernel: both nets through their act tables */
#define EVX_FWD_TARGET_ACT_TABLE 4  /* x_expand_kernel + qact3h_kernel SAVE (online), qact3h_kernel (target) */
#define EVX_FWD_TARGET_ACT_FC 5     /* qfc1_kernel + qfc23_kernel (online), qact3h_kernel (target) */
#define EVX_FWD_ACT_BF16 6          /* qact_kernel: 128-row tiles */
#define EVX_FWD_ACT_64 7            /* qact3h_kernel: 64-row tiles */
#define EVX_FWD_ACT_PERSISTENT 8    /* qact3p_kernel on act_grid workgroups, then qact3h_rest_kernel */
#define EVX_FWD_ACT_GROUPED 9       /* qact3h_kernel's grouped instantiation (blockIdx.y = net) */
/* Every launch of one evx_qmlp_forward / _forward2 / _forward2_g / _stat / _stat_x / _act / _act64 /
 * _act_g call. The tile and grid fields are 0 where the route has no such launch. */
typedef struct {
    int32_t route;        /* EVX_FWD_* */
    int32_t fc1_rows;     /* rows per qfc1 tile: 64 or 128 (0: no qfc1 launch) */
    int32_t fc1_cols;     /* fc1 columns per workgroup: 128, 256 or 512 */
    int32_t fc23_rows;    /* rows per qfc23 tile: 32 or 64 (0: no qfc23 launch) */
    int32_t drop_mode;    /* the dropout instantiation: 0 none, 1 the hash, 2 an explicit mask */
    int32_t drop_mode1;   /* the same of the second problem (the routes with a target act) */
    int32_t x_expand;     /* 1: x_expand_kernel writes the first problem's X by its own launch */
    int32_t act_grid;     /* persistent act: workgroups of qact3p_kernel */
    int32_t rest_grid;    /* persistent act: workgroups of qact3h_rest_kernel */
    int32_t rest_listed;  /* persistent act: 1 when the rest runs the tiles listed in act_ws, 0: every row */
} evx_qmlp_fwd_plan;
/* The plan of evx_qmlp_forward2 with these arguments (obs1 = p1 = out1 = NULL: of evx_qmlp_forward;
 * nets >= 1: of evx_qmlp_forward2_g; nets = 0: the single-net entry points), decided by the function
 * the launchers themselves switch on: no launch, no device call (pointers are only tested for NULL).
 * An argument error the call would report comes back as the same code with the same text. */
int evx_qmlp_fwd_plan_query(const evx_layout *lay, int32_t n, const evx_obs *obs0, const evx_qmlp_params *p0,
                            const evx_qmlp_dropout *drop0, const evx_qmlp_fwd_out *out0, const evx_obs *obs1,
                            const evx_qmlp_params *p1, const evx_qmlp_dropout *drop1, const evx_qmlp_fwd_out *out1,
                            int32_t nets, evx_qmlp_fwd_plan *plan);
/* The same of evx_qmlp_act (kernel64 != 0: evx_qmlp_act64; nets >= 1: evx_qmlp_act_g) on a device of
 * ncu compute units; ncu <= 0 asks the current device (the only device call). */
int evx_qmlp_act_plan_query(const evx_layout *lay, const evx_obs *obs, int32_t n, const evx_qmlp_params *p,
                            const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out, int32_t nets,
                            int32_t kernel64, int32_t ncu, evx_qmlp_fwd_plan *plan);

/* ---- A population of independent learners (evacx/population.py): member k owns a contiguous block
 * of envs, so its rows are a block of every row buffer, not a stride through it. */
/* The route of evx_qmlp_act_gb, appended to the EVX_FWD_* values above (an enumerator: the #define
 * list stays the set of routes the single-net and per-robot entries take). */
enum { EVX_FWD_ACT_GROUPED_BLOCKED = 10 /* qact3h_gb_kernel (blockIdx.y = net, its rows one block) */ };
/* The blocked grouped act: net g reads obs rows [g n, (g + 1) n) and writes the same rows of q /
 * actions (n rows per net, even): the single-net act of that block through net g with dropout row0
 * = g n, exploration epsilon[g] (host array [nets]; out->epsilon is not read) and epsilon draws
 * counted from out->act_offset + g n. x3 parameters in the [nets] layout above. No act table, no
 * permutation, no act_ws. -22 before any launch: a NULL required pointer, nets outside 1..64, n odd,
 * an epsilon that is not finite, and what evx_qmlp_act_g refuses. */
int evx_qmlp_act_gb(const evx_layout *lay, const evx_obs *obs, int32_t n, int32_t nets, const evx_qmlp_params *p,
                    const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out, const float *epsilon, void *stream);
/* Its plan (as evx_qmlp_act_plan_query: the launcher's own decision, nothing launched, no device call). */
int evx_qmlp_act_gb_plan_query(const evx_layout *lay, const evx_obs *obs, int32_t n, int32_t nets,
                               const evx_qmlp_params *p, const evx_qmlp_dropout *drop, const evx_qmlp_fwd_out *out,
                               const float *epsilon, evx_qmlp_fwd_plan *plan);
/* `nets` replay rings of rp->capacity slots each as one allocation [nets][capacity] per array of rp
 * (ring k's arrays start k * capacity slots after ring 0's, which rp points at). Every ring takes n
 * rows per push, so pos and size are common to them.
 * evx_replay_push_blocks: evx_replay_push_term of rows [k n, (k + 1) n) of s / s2 / s2_term / a into
 * ring k at pos, for every k in one launch: row k n + i goes to slot (pos + i) mod capacity with the
 * reward and done flag of env (k n + i) / agents_per_env, s2_term (may be NULL) where that env is done.
 * evx_replay_sample_blocks: rows [k B, (k + 1) B) of the outputs are what
 * evx_replay_sample(ring k, size, B, seed, offset + k B) draws, for every k in one launch.
 * -22 before any launch: a NULL required pointer, nets outside 1..64, n or B odd, a capacity that
 * does not hold n, n no multiple of agents_per_env, pos outside [0, capacity), size outside
 * [1, capacity], B > size. */
int evx_replay_push_blocks(const evx_replay *rp, const evx_obs *s, const evx_obs *s2, const evx_obs *s2_term,
                           const int32_t *a, const double *r_env, const uint8_t *done_env, int32_t n, int32_t nets,
                           int32_t agents_per_env, int64_t pos, void *stream);
int evx_replay_sample_blocks(const evx_replay *rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                             uint64_t offset, evx_obs *s, evx_obs *s2, int32_t *a, float *r, uint8_t *done,
                             void *stream);
/* The population's learner options: each member its own n-step depth, Huber delta and Polyak rate
 * (host arrays [nets], passed to the kernels by value as evx_qmlp_act_gb's epsilons are).
 * evx_replay_sample_nstep_blocks: evx_replay_sample_blocks and evx_replay_nstep in one launch. Row
 * k B + i draws ring k's slot j0 as evx_replay_sample_blocks does, takes s and a from it and follows
 * evx_replay_nstep's chain on ring k with n_step[k] and gamma[k] over the live range [base, base +
 * count) mod capacity (common to the rings; successor of slot j: (j + stride) mod capacity): r = the
 * discounted return, s2 / done = the chain's last slot's, gamma_row = gamma[k]^L, len = L (int32
 * [nets][B], may be NULL), idx_out = j0 (int64 [nets][B], ring-local, may be NULL). All f32, R + g r
 * a multiply and an add. Every n_step = 1: evx_replay_sample_blocks bit for bit, gamma_row = gamma[k],
 * len = 1. A stride beyond the ring is taken as the capacity (no successor lies inside the range).
 * -22 before any launch: a NULL required pointer, nets outside 1..64, B odd, size outside
 * [1, capacity], B > size, count outside [0, capacity], base outside [0, capacity), stride < 1, an
 * n_step outside 1..EVX_NSTEP_MAX, a gamma that is not finite. */
int evx_replay_sample_nstep_blocks(const evx_replay *rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                                   uint64_t offset, int64_t base, int64_t count, int64_t stride,
                                   const int32_t *n_step, const float *gamma, evx_obs *s, evx_obs *s2, int32_t *a,
                                   float *r, uint8_t *done, float *gamma_row, int32_t *len, int64_t *idx_out,
                                   void *stream);
/* evx_td_loss_opt with a Huber delta per net: huber_delta [nets] on the host (0: that net's squared
 * error) in place of opt->huber_delta, which is not read; opt may be NULL (no sel, no gamma_row).
 * Equal deltas give evx_td_loss_opt bit for bit. -22 before any launch: a NULL required pointer,
 * nets outside 1..64, a delta that is negative or not finite, and what evx_td_loss_opt refuses. */
int evx_td_loss_opt_nets(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                         const uint8_t *done, float gamma, int32_t B, int32_t nets, const float *w, float *dQ,
                         float *loss, float *td_abs, float *zero, int64_t nzero, float *ws, int64_t ws_floats,
                         const evx_td_opts *opt, const float *huber_delta, void *stream);
/* evx_qmlp_polyak_pack3 of every net in one launch: p / t [nets][evx_qmlp_nparams()], the operand
 * buffers in the [nets] layout above; tau / one_minus_tau [nets] on the host (one_minus_tau[g] =
 * (float)(1.0 - (double)tau[g])). Net g with tau[g] = 0 is skipped: its target parameters and
 * operand buffers keep their bits, so members with a hard target copy and members with a soft one
 * share the launch. Per net evx_qmlp_polyak_pack3 bit for bit. -22 before any launch: a NULL
 * required pointer, nets outside 1..64, a tau outside [0, 1], a one_minus_tau that is not finite,
 * w1o / w1ol or w2t / w2tl given singly. */
int evx_qmlp_polyak_pack3_g(const float *p, float *t, const float *tau, const float *one_minus_tau, uint16_t *w1b,
                            uint16_t *w1l, float *b1c, uint16_t *w2b, uint16_t *w2l, uint16_t *w2t, uint16_t *w2tl,
                            uint16_t *w1o, uint16_t *w1ol, int32_t nets, void *stream);
/* Exploit step of population-based training: members take other members' blocks of [members][...]
 * arrays, every array and every receiver in one launch. One evx_member_buf describes one array:
 * member k's block is bytes [0, bytes) at base + k * stride_bytes. */
typedef struct {
    void *base;           /* member 0's block (device) */
    int64_t stride_bytes; /* from one member's block to the next */
    int64_t bytes;        /* of a block that are copied (<= stride_bytes) */
} evx_member_buf;
/* For every member k with src[k] != k and every buffer b: bytes [0, bytes) of base + k * stride_bytes
 * <- the same bytes of base + src[k] * stride_bytes. bufs [nbufs] and src [members] are host arrays,
 * passed to the kernel by value as evx_qmlp_act_gb's epsilons are. One launch, grid (chunk, receiver,
 * buffer): 16 bytes per lane where the two blocks are congruent mod 16 (4-byte words before and
 * after the aligned part), 4 bytes per lane otherwise; members that keep their block, the donors
 * among them, and every byte outside the blocks are not written. The identity map returns 0 without
 * a launch. -22 before any launch: a NULL pointer (bufs, src, a base), members outside 1..64, nbufs
 * outside 1..32, a src[k] outside 0..members - 1, a donor that is itself replaced (src[src[k]] !=
 * src[k]: a read / write race inside the launch), a base, stride_bytes or bytes that is no multiple
 * of 4, bytes negative or > stride_bytes. */
int evx_copy_members(const evx_member_buf *bufs, int32_t nbufs, const int32_t *src, int32_t members, void *stream);

/* ---- QMIX mixer (runners/train_qmix.py:39-54 MixingNetwork, loss :78-104) for n <= 16 agents:
 * Q / Qt [n][B][A] (evx_qmlp_forward2_g), act [n][B], rew / done [B]; mix / mix_t the online /
 * target mixer flat in state_dict order (fc1_weight [n][32], fc1_bias [32], fc2_weight [32][1],
 * fc2_bias [1]: evx_qmix_nparams(n)). Writes dQ [n][B][A] (d loss / d Q at the taken actions),
 * the online mixer's gradient and loss[0] = mse; part: evx_qmix_part_floats(B, n) floats of
 * scratch; zero[0..nzero) (the agents' gradients) is cleared in the same launch. */
int32_t evx_qmix_nparams(int32_t n);
int64_t evx_qmix_part_floats(int32_t B, int32_t n);
int evx_qmix_loss(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                  const uint8_t *done, float gamma, int32_t B, int32_t n, const float *mix, const float *mix_t,
                  float *dQ, float *mix_grad, float *loss, float *part, float *zero, int64_t nzero, void *stream);
/* evx_qmix_loss with the TD options (evx_td_opts, layout unchanged) applied to the mixed value: sel
 * [n][B] (agent-major like act), gamma_row [B] (one discount per joint row), huber_delta one value;
 * opt may be NULL. td_abs [B] (may be NULL) gets |d|. Per joint row b, all f32, in the order of
 * evx_qmix_loss:
 *   q_i   = Q[i][b][act[i][b]]
 *   j*_i  = sel ? clamp(sel[i][b], 0, A - 1) : the maximum of Qt[i][b][.];   qt_i = Qt[i][b][j*_i]
 *   tot_t = target mixer(qt),  tot = online mixer(q)
 *   y     = rew[b] + (gamma_row ? gamma_row[b] : gamma) * tot_t * (done[b] ? 0 : 1)
 *   d     = tot - y;  td_abs[b] = |d|
 *   huber_delta = 0:  l = d * d,  dqt = 2 d / B
 *   huber_delta > 0:  l = |d| <= delta ? 0.5 (d * d) : delta (|d| - 0.5 delta),  dqt = min(max(d, -delta), delta) / B
 *   loss = mean(l); the backward through the online mixer from dqt, the mixer's gradient and the
 *   clear of zero as in evx_qmix_loss. With Double-Q every agent bootstraps from its own greedy
 *   action and the monotone target mixer combines those values; the Huber loss and its clamp act
 *   on the team's TD error d, not per agent.
 * opt = NULL and td_abs = NULL: evx_qmix_loss bit for bit (the same kernel, the options compiled
 * out there). part, its summation order and the LDS footprint are evx_qmix_loss's.
 * B <= 0: 0, nothing written. -22 before any launch (evx_qmix_last_error): what evx_qmix_loss
 * refuses (n outside 1..16, A outside 1..64, a NULL required pointer), a huber_delta that is
 * negative or not finite, a gamma that is not finite. */
int evx_qmix_loss_opt(const float *Q, const float *Qt, int32_t A, const int32_t *act, const float *rew,
                      const uint8_t *done, float gamma, int32_t B, int32_t n, const float *mix, const float *mix_t,
                      float *dQ, float *mix_grad, float *loss, float *part, float *zero, int64_t nzero,
                      const evx_td_opts *opt, float *td_abs, void *stream);
const char *evx_qmix_last_error(void);

/* ---- Episode statistics (csrc/episode.hip). The reference's training loop adds each step's
 * reward into total_reward on the host and logs the episode's return, evacuation_rate and
 * death_rate when done comes back (runners/train_dqn.py:129-161; evaluate_strategies.py:47-77
 * does the same per strategy). The vectorised envs reset inside the step launch, so the same
 * bookkeeping runs on the device from the step's outputs. Every array is per env ([E] unless
 * noted): an env's numbers depend on its own step sequence only, never on the order in which
 * envs, groups or streams run, and nothing is added with float atomics. A part of the envs
 * (VecEnv.split) is a descriptor whose pointers are offset to its first env and whose E is
 * its env count. */
typedef struct {
    int32_t E;
    int32_t tab_slots;     /* K: episodes per env the episode table holds (0 = no table) */
    /* the episode in progress */
    double *ret;           /* sum of its rewards so far, f64 adds in step order */
    int32_t *len;          /* its steps so far */
    /* the window: episodes folded since the last clear */
    int64_t *w_n, *w_len, *w_evac, *w_dead; /* count, sum of lengths, of evacuated, of dead */
    double *w_ret, *w_ret2;                 /* sum of returns, of squared returns (episode order) */
    double *w_min, *w_max;                  /* smallest / largest return (+inf / -inf when empty) */
    /* the last finished episode */
    double *last_ret;
    int32_t *last_len, *last_evac, *last_dead;
    int64_t *n_total;      /* episodes finished since evx_episode_init (never cleared) */
    /* optional episode table [E][K]: the env's episode with lifetime index k < K in slot k */
    double *tab_ret;
    int32_t *tab_len, *tab_evac, *tab_dead;
} evx_episodes;

/* One row of evx_episode_reduce: the window summed over a set of envs. */
typedef struct {
    int64_t episodes, len_sum, evac_sum, dead_sum;
    double ret_sum, ret2_sum, ret_min, ret_max;
    int64_t remaining;     /* envs of the row whose lifetime count is < cap (0 when cap <= 0) */
    int64_t no_episode;    /* envs of the row that have not finished an episode yet */
} evx_episode_row;

/* envs one pass of a reduce workgroup covers (its thread count) */
#define EVX_EPISODE_REDUCE_SPAN 1024

/* Everything zeroed: no episode in progress, empty window (min +inf, max -inf), lifetime 0. */
int evx_episode_init(const evx_episodes *ep, void *stream);
/* One step of every env of ep, one launch: ret += reward[e] (the reference's total_reward +=
 * reward), len += 1; where done[e], the episode is folded into the window (w_ret2 += ret * ret,
 * not contracted), the last-episode slots and the table, with counts[2e], counts[2e + 1] its
 * terminal evacuated and dead (evx_step_out.counts), the lifetime count is bumped and ret, len
 * start again from 0. cap > 0: an episode whose lifetime index (n_total before the bump) is >= cap
 * stays out of the window, so the window holds exactly the first cap episodes of every env. */
int evx_episode_update(const evx_episodes *ep, const double *reward, const uint8_t *done, const int32_t *counts,
                       int64_t cap, void *stream);
/* Drops the episode in progress (ret = 0, len = 0) of the envs with mask[e] != 0 (NULL: all):
 * for envs reset from outside the step (evx_env_reset). */
int evx_episode_discard(const evx_episodes *ep, const uint8_t *mask, void *stream);
/* The window summed over envs into out[0 .. n_layouts]: row l < n_layouts over the envs with
 * layout_idx[e] == l (NULL: every env is of layout 0), row n_layouts over all envs. Integer
 * fields are exact. The f64 sums of a row are added in one fixed order -- the same bits on every
 * run and however the updates were sliced: thread t of the row's workgroup (EVX_EPISODE_REDUCE_SPAN
 * threads) adds the row's envs t, t + SPAN, t + 2 SPAN, ... in ascending order onto 0.0 (envs of
 * other layouts are skipped), then the thread sums are added pairwise, s[t] = s[t] + s[t + h] for
 * h = SPAN/2, SPAN/4, ..., 1; the row's sum is s[0]. clear != 0: the per-env window arrays are
 * emptied by a second launch of the same call; the episode in progress, the last-episode slots,
 * the table and the lifetime count stay. Any E >= 1. (The order is implemented once, in
 * csrc/evx_reduce.h, for this reduce, evx_health_reduce and evx_vprobe_reduce.) */
int evx_episode_reduce(const evx_episodes *ep, const int32_t *layout_idx, int32_t n_layouts, int64_t cap,
                       evx_episode_row *out, int32_t clear, void *stream);
const char *evx_episode_last_error(void);

/* ---- Terminal health (csrc/health.hip): EvacuationEnv.get_performance_metrics()'s avg_health
 * and min_health (envs/evacuation_env.py:290-309) of every finished episode, taken on the device
 * from the persons' pk / health as the step left them and before any reset (step with resets
 * apart, evx_health_update, then evx_env_reset with the done mask). Per env, like evx_episodes:
 * an env's numbers depend on its own episodes only, and a part of the envs is a descriptor
 * whose pointers are offset to its first env. The lifetime count is its own, so the result does
 * not depend on whether the update runs before or after evx_episode_update. */
typedef struct {
    int32_t E;
    int32_t tab_slots;     /* K: episodes per env the health table holds (0 = no table) */
    int64_t *n_total;      /* episodes seen since evx_health_init (never cleared) */
    /* the window: episodes folded since the last clear */
    int64_t *w_n;          /* episodes */
    int64_t *w_has;        /* episodes among them with alive > 0 (the ones that have an avg_health) */
    int64_t *w_alive;      /* sum of alive */
    double *w_avg;         /* sum of avg_health over the episodes that have one, in episode order */
    double *w_min;         /* sum of min_health, in episode order */
    double *w_lo;          /* smallest min_health (+inf when empty) */
    /* the last finished episode */
    double *last_avg, *last_min;
    int32_t *last_alive;
    /* optional table [E][K]: the env's episode with lifetime index k < K in slot k */
    double *tab_avg, *tab_min;
    int32_t *tab_alive;
} evx_health;

/* One row of evx_health_reduce: the window summed over a set of envs. */
typedef struct {
    int64_t episodes, health_episodes, alive_sum;
    double avg_sum, min_sum, min_min;
} evx_health_row;

/* the largest P evx_health_update takes (the env's own bound) */
#define EVX_HEALTH_MAX_P 16383

/* Everything zeroed: empty window (w_lo +inf), last-episode slots 0, lifetime 0. */
int evx_health_init(const evx_health *h, void *stream);
/* One launch, one wave per env of h; an env with done[e] == 0 is left untouched. For the others,
 * from pk[e][0..P) and health[e][0..P) (any [E][P] arrays; P 1..EVX_HEALTH_MAX_P):
 *   alive      = persons whose dead bit (pk bit 25) is clear (evacuated persons count);
 *   min_health = the smallest health among them, 100.0 when there are none;
 *   avg_health = np.mean of their healths in person order, bit for bit: the compacted list is
 *                cut into consecutive chunks of 8192, each chunk is summed with numpy's pairwise
 *                sum (n < 8 a plain loop from 0.0; n <= 128 eight strided accumulators combined
 *                as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order; else split at
 *                n/2 rounded down to a multiple of 8), the chunk sums are added left to right
 *                onto the first and the total is divided by alive; NaN when alive == 0.
 * The three values go to the last-episode slots, to table slot n_total[e] if it is < tab_slots,
 * and into the window unless cap > 0 and n_total[e] >= cap (evx_episode_update's rule); then
 * n_total[e] is bumped. No atomics, no host sync. */
int evx_health_update(const evx_health *h, const int32_t *pk, const double *health, int32_t P, const uint8_t *done,
                      int64_t cap, void *stream);
/* The window summed over envs into out[0 .. n_layouts] (rows as in evx_episode_reduce) in the same
 * fixed order: thread t of EVX_EPISODE_REDUCE_SPAN adds the row's envs t, t + SPAN, ... ascending
 * onto 0.0, then the thread sums are added pairwise, s[t] = s[t] + s[t + h] for h = SPAN/2, ..., 1.
 * Integer fields are exact. clear != 0: the window arrays are emptied by a second launch. */
int evx_health_reduce(const evx_health *h, const int32_t *layout_idx, int32_t n_layouts, evx_health_row *out,
                      int32_t clear, void *stream);
const char *evx_health_last_error(void);

/* ---- Evacuation timelines and tracked persons (csrc/timeline.hip): what the reference's recorded
 * evaluation episode keeps (DQNTrainingVisualizer, utils/visualization.py) -- evacuated, dead and
 * avg_health after every step, the evacuation-time and death-time distributions from the per-step
 * count deltas, and selected persons step by step -- over every episode of every env. All arrays
 * are the caller's device arrays. Everything added across envs is an integer (health in fixed
 * point at 2^-20), so the result does not depend on the order of the adds; no float atomics. */
typedef struct {
    int32_t E;
    int32_t T;             /* slots per row: slot s holds episode step s + 1 */
    int32_t n_rows;        /* layout rows (an env's row is layout_idx[e], 0 without layout_idx) */
    int32_t n_trk;         /* tracked persons (0: no trace, the trk_* pointers may be NULL) */
    /* per env [E] */
    int32_t *t;            /* steps of the episode in progress */
    int32_t *p_evac, *p_dead; /* counts after that episode's previous step */
    int64_t *n_total;      /* episodes finished since evx_timeline_init (the timeline's own count) */
    /* per row and slot [n_rows][T] */
    int64_t *evac, *dead;  /* persons newly evacuated / newly dead at that step */
    int64_t *ended;        /* episodes that ended at that step */
    int64_t *seen;         /* episodes recorded at that step */
    int64_t *alive;        /* sum over those episodes of the persons whose dead bit (pk bit 25) is clear */
    int64_t *health_q;     /* sum over those persons of llrint(health * 2^20), round half even */
    int64_t *late;         /* [n_rows][4]: evac, dead, ended, steps at episode steps beyond T */
    int64_t *bad_health;   /* [1]: not-dead persons with |health| > 128 (or NaN), left out of alive and health_q */
    /* optional trace of n_trk persons over their env's first episode */
    int32_t *trk_env, *trk_person; /* [n_trk], input; clamped into 0..E-1 and 0..P-1 */
    uint32_t *trk_pk;      /* [T + 1][n_trk]: slot 0 the state after the reset, slot t after step t */
    double *trk_health;    /* [T + 1][n_trk] */
    int32_t *trk_len;      /* [n_trk]: slots written */
} evx_timeline;

/* Zeroes every array of tl but trk_env / trk_person (one launch). */
int evx_timeline_init(const evx_timeline *tl, void *stream);
/* One step of every env of tl from the step's counts[2e], counts[2e + 1] (evacuated, dead so far)
 * and done[e] (evx_step_out). With s = t[e] the env's slot and row = layout_idx[e] (NULL: 0;
 * clamped into 0..n_rows-1), an episode whose lifetime index n_total[e] is < cap (cap <= 0: every
 * episode; evx_episode_update's rule) adds to [row][s]: evac += counts[2e] - p_evac[e],
 * dead += counts[2e + 1] - p_dead[e], ended += done[e] != 0, seen += 1 and, with pk / health
 * ([E][P] as the step left them, before any reset; P 1..EVX_HEALTH_MAX_P), alive and health_q over
 * the persons whose dead bit is clear and whose |health| <= 128; the others of them are counted in
 * bad_health. s >= T: the first four go to late[row] instead. Then t, p_evac, p_dead take the step,
 * or, where done[e], start again from 0 and n_total[e] is bumped. pk = health = NULL (callers whose
 * resets are fused into the step) leaves alive and health_q alone.
 * n_trk > 0 (needs pk / health): a first launch of the same call writes every tracked person's pk
 * and health to trace slot t[e] + 1 (<= T) while n_total[e] == 0. The update launch runs one wave
 * per env, 8 envs per workgroup; envs of a workgroup on the same (row, slot) are combined in LDS
 * before one returnless 64-bit integer atomic add per field and destination. -22 with a message,
 * before any launch: a NULL descriptor, required array, counts or done; E < 1 or T < 1;
 * n_rows < 1; P out of range; pk without health or health without pk; n_trk > 0 with a NULL trace
 * array or without pk. */
int evx_timeline_update(const evx_timeline *tl, const int32_t *counts, const uint8_t *done, const int32_t *layout_idx,
                        const int32_t *pk, const double *health, int32_t P, int64_t cap, void *stream);
/* Trace slot 0 of the tracked persons whose env has not finished an episode: the state after the
 * first reset. Nothing is launched with n_trk == 0. */
int evx_timeline_trace0(const evx_timeline *tl, const int32_t *pk, const double *health, int32_t P, void *stream);
const char *evx_timeline_last_error(void);

/* ---- Spatial maps (csrc/spatial.hip): where an evacuation happened -- per layout row and grid
 * cell, how many persons arrived, stood still, left through an exit or died there, and where the
 * robots spent their steps -- over every counted episode of every env. The reference keeps one
 * per-env diagnostic (People.thmap) and aggregates nothing. All arrays are the caller's device
 * arrays; every accumulator is an integer count, so the result does not depend on the order of the
 * adds and there are no float atomics. The grid is the padded one of the env kernels:
 * GX = L + 2, GY = W + 2, cell = x * GY + y, G = GX * GY. */
typedef struct {
    int32_t E;
    int32_t P;             /* persons per env, 1..EVX_HEALTH_MAX_P */
    int32_t R;             /* robots per env, >= 0 */
    int32_t GX, GY;        /* 1..4096 each */
    int32_t n_rows;        /* layout rows (an env's row is layout_idx[e], 0 without layout_idx) */
    uint32_t *prev;        /* [E][P]: each env's pk as of the previous state */
    int64_t *n_total;      /* [E]: episodes finished since evx_spatial_init (the maps' own count) */
    /* per row and cell [n_rows][G] */
    int64_t *arrive;       /* live persons that stand on a cell other than the one before the step */
    int64_t *stall;        /* live persons that stand on the cell they stood on before the step */
    int64_t *evac;         /* persons that became safe at the step, at the cell they are on */
    int64_t *died;         /* persons that died at the step */
    int64_t *robot;        /* robot positions after the step */
    int64_t *steps;        /* [n_rows]: env-steps folded */
    int64_t *bad;          /* [1]: persons and robots whose cell lies outside the grid, left out of every map */
} evx_spatial;

/* EVX_SPATIAL_*: how evx_spatial_update accumulates the two dense maps (arrive, stall) */
#define EVX_SPATIAL_LDS 1   /* one launch: both maps of the whole grid as u32 counters in LDS */
#define EVX_SPATIAL_BANDS 2 /* the grid cut into x-bands that fit, one workgroup column per band, and a
                               second launch that takes the step (prev, n_total) */

/* The launch shape of evx_spatial_update, as the launcher itself decides it (evx_spatial_plan). */
typedef struct {
    int32_t route;         /* EVX_SPATIAL_* */
    int32_t bands;         /* x-bands (grid.y of the update launch); 1 on EVX_SPATIAL_LDS */
    int32_t band_w;        /* columns (x) per band */
    int32_t band_cells;    /* band_w * GY: counters per map in LDS */
    int32_t lds_bytes;     /* dynamic LDS of one workgroup: 64 + 8 * band_cells, at most 160 KiB */
    int32_t envs_per_wg;   /* envs one workgroup folds before it flushes its counters (grid.x = ceil(E / this)) */
    int32_t threads;       /* threads per workgroup; one wave takes one env at a time */
    int32_t launches;      /* 1, or 2 with bands */
} evx_spatial_launch;

/* Zeroes prev, n_total, the five maps, steps and bad (one launch). */
int evx_spatial_init(const evx_spatial *sp, void *stream);
/* prev[e][.] = pk[e][.] for the envs with mask[e] != 0 (mask == NULL: every env), one launch. Call
 * it after the first reset and after every masked reset: the state a reset writes is where the next
 * episode's persons start, not a move. pk is typed as evx_timeline_update takes it. */
int evx_spatial_sync(const evx_spatial *sp, const int32_t *pk, const uint8_t *mask, void *stream);
/* One step of every env from pk [E][P] as the step left it, before any reset, and robots [E][R]
 * (evx_state.robots: (u16)x | (u16)y << 16, where the robots stand after the step; evx_state.view
 * is only the centre of robot 0's observation and may lag behind). For env e:
 *   row = clamp(layout_idx[e], 0, n_rows - 1), 0 with layout_idx == NULL;
 *   the env is counted iff cap <= 0 || n_total[e] < cap (evx_episode_update's rule).
 * For every person i of a counted env, with old = prev[e][i], cur = pk[e][i], x = v & 0xfff,
 * y = (v >> 12) & 0xfff, safe = bit 24, dead = bit 25, live = neither bit, cell(v) = x * GY + y:
 *   old not live: nothing (safe and dead are absorbing);
 *   cur outside the grid (x >= GX || y >= GY): bad += 1, nothing else;
 *   otherwise exactly one map takes 1 at [row][cell(cur)]: evac if cur is safe (safe wins over
 *   dead), else died if cur is dead, else arrive if cell(cur) != cell(old), else stall.
 * For every robot of a counted env robot[row][cell] += 1, or bad += 1 outside the grid; and
 * steps[row] += 1. Then, for every env, counted or not: prev[e][.] = pk[e][.], and
 * n_total[e] += 1 where done[e].
 * occupancy = arrive + stall is the live persons per cell after the step; flow = arrive + evac is
 * the persons that entered a cell, exact while every newly safe person also moved.
 * arrive and stall are counted in LDS: a workgroup of 1024 threads folds envs_per_wg envs, one wave
 * per env at a time and row by row, into u32 counters (envs_per_wg * P < 2^32, so no input can
 * overflow one) and flushes the non-zero ones with returnless 64-bit atomic adds; evac, died and
 * robot, which take at most one add per person and episode or R per env-step, go straight to
 * 64-bit atomics. A grid whose two maps exceed 160 KiB of LDS is cut into x-bands
 * (EVX_SPATIAL_BANDS): workgroup (s, b) folds the persons of share s whose x lies in band b, band 0
 * also the robots, bad and steps, and a second launch writes prev and n_total.
 * -22 with a message, before any launch: a NULL descriptor or descriptor array; E < 1; P outside
 * 1..EVX_HEALTH_MAX_P; R < 0; GX or GY outside 1..4096; n_rows < 1; NULL pk or done; NULL robots
 * with R > 0. */
int evx_spatial_update(const evx_spatial *sp, const int32_t *pk, const int32_t *robots, const uint8_t *done,
                       const int32_t *layout_idx, int64_t cap, void *stream);
/* The route and launch shape evx_spatial_update takes for this grid and P, from the function the
 * launcher itself calls; no launch and no device call. -22 for sizes the update refuses. */
int evx_spatial_plan(int32_t GX, int32_t GY, int32_t P, int32_t n_rows, evx_spatial_launch *plan);
const char *evx_spatial_last_error(void);

/* ---- Learner diagnostics (csrc/lstats.hip): what Double-Q, the Huber loss and the soft target
 * exist to control -- the Q-values, targets and TD errors of the sampled batches, the loss and the
 * pre-clip gradient norm -- accumulated on the device over a window of learn steps, and a value
 * probe that pairs the act's Q at an episode's first step with the discounted return the episode
 * then obtains. Neither has a counterpart in the reference (its loop prints the episode reward).
 * Both only read the learner's and the env's buffers. All arrays are the caller's device arrays. */
#define EVX_LSTATS_MAX_A 8
#define EVX_LSTATS_TD_BUCKETS 48
/* doubles one 256-row block leaves in the workspace: the sums of q, qmax, y, d, |d|, d d, rew,
 * then the largest |d|, the largest qmax and the smallest Q */
#define EVX_LSTATS_WS_FIELDS 10
typedef struct {
    int32_t nets;          /* 1..64 */
    int32_t A;             /* actions per row, 1..EVX_LSTATS_MAX_A */
    /* per net [nets] */
    int64_t *steps;        /* updates (learn steps) in the window */
    int64_t *steps_bad;    /* those whose loss or norm was not finite */
    int64_t *rows;         /* batch rows seen */
    int64_t *rows_bad;     /* those with a non-finite q, qmax or y: counted here and nowhere else */
    int64_t *n_done;       /* good rows with done != 0 */
    int64_t *n_greedy;     /* good rows whose action is the first maximum of their Q row */
    int64_t *n_clipped;    /* good steps with max_norm > 0 and norm > max_norm */
    int64_t *act_hist;     /* [nets][EVX_LSTATS_MAX_A]: good rows by (clamped) action */
    int64_t *td_hist;      /* [nets][EVX_LSTATS_TD_BUCKETS]: good rows by the octave of |d| */
    double *s_q, *s_qmax, *s_y, *s_d, *s_absd, *s_d2, *s_rew; /* sums over good rows */
    double *s_loss, *s_norm;                                  /* sums over good steps */
    double *max_absd, *max_q, *min_q, *max_loss, *max_norm;   /* -inf (min_q: +inf) when empty */
} evx_lstats;

/* doubles of workspace one evx_lstats_update of B rows per net needs:
 * nets * ceil(B / 256) * EVX_LSTATS_WS_FIELDS (0 when B < 1 or nets < 1) */
int64_t evx_lstats_ws_doubles(int32_t B, int32_t nets);
/* Empties the window: counts 0, sums 0.0, max_* -inf, min_q +inf (one launch). */
int evx_lstats_init(const evx_lstats *ls, void *stream);
/* One learn step's batch folded into the window. Net g's rows are [g B, (g + 1) B) of Q / Qt
 * ([.][A] f32), act, rew, done, opt->sel, opt->gamma_row and d_out (the blocked layout of
 * evx_qmlp_forward2_g and evx_td_loss_opt). Per row, all f32 and not contracted -- the TD kernels'
 * expressions (above evx_td_opts), without the importance weights; opt = NULL: no options,
 * opt->huber_delta is ignored:
 *   a    = clamp(act[i], 0, A - 1);  q = Q[i][a]
 *   qmax, jmax = the first maximum of Q[i][0..A-1] (strict > while scanning j = 1..A-1);
 *   qmin likewise the first minimum (strict <)
 *   j*   = sel ? clamp(sel[i], 0, A - 1) : the first maximum's index of Qt[i][.]
 *   y    = rew[i] + ((gamma_row ? gamma_row[i] : gamma) * Qt[i][j*]) * (done[i] ? 0 : 1)
 *   d    = q - y;   bad = !(isfinite(q) && isfinite(qmax) && isfinite(y))
 * Every row counts in rows; a bad row in rows_bad and nowhere else; a good row adds the f64 values
 * of q, qmax, y, d, |d|, d d (the f64 product of the f64 values) and rew to the sums, done != 0 to
 * n_done, act[i] == jmax to n_greedy, 1 to act_hist[a], 1 to td_hist[k] with
 * k = min(max((bits(|d|) >> 23) - 103, 0), 47) (bucket k >= 1: 2^(k-24) <= |d| < 2^(k-23); bucket 0:
 * everything below 2^-23; bucket 47: everything from 2^23), and |d|, qmax, qmin to max_absd, max_q,
 * min_q. d_out (optional, [nets][B]): the row's d, NaN for a bad row.
 * Summation order of every f64 sum: net g's rows are cut into blocks of 256; thread t of a block
 * holds row t's value, 0.0 for a bad row or a row beyond B; s[t] = s[t] + s[t + h] for h = 128, 64,
 * ..., 1; the block sums are added in ascending block order onto 0.0 and that step total is added
 * to the window's accumulator. No float atomics; the integer counts are added with integer atomics.
 * Two launches: the rows kernel leaves each block's EVX_LSTATS_WS_FIELDS doubles in ws
 * (ws_doubles >= evx_lstats_ws_doubles(B, nets)), then one workgroup per net adds them in order.
 * That second launch also takes the step: steps += 1; with l = loss[g], n = norm[g] (f32 device
 * scalars per net, each optional; a NULL one leaves its fields alone and counts as finite): both
 * finite: s_loss += l, s_norm += n, max_loss, max_norm, n_clipped += (max_norm > 0 && n > max_norm);
 * otherwise steps_bad += 1.
 * -22 with a message, before any launch: a NULL descriptor, descriptor array, Q, Qt, act, rew, done
 * or ws; nets outside 1..64; A outside 1..EVX_LSTATS_MAX_A; B < 1; nets * B beyond 2^31 - 1; ws_doubles
 * too small; gamma not finite. */
int evx_lstats_update(const evx_lstats *ls, const float *Q, const float *Qt, const int32_t *act, const float *rew,
                      const uint8_t *done, float gamma, int32_t B, const evx_td_opts *opt, const float *loss,
                      const float *norm, float max_norm, float *d_out, double *ws, int64_t ws_doubles, void *stream);
const char *evx_lstats_last_error(void);

/* The value probe, per env [E] like evx_episodes (a part of the envs is a descriptor whose pointers
 * are offset to its first env): at the first step of every episode the mean over the env's R robots
 * of the Q-value the act computed for the action taken is kept with the discounted return the
 * episode goes on to obtain; at done the pair is folded into the window. */
typedef struct {
    int32_t E;
    int32_t R;             /* robots (act rows) per env */
    int32_t A;             /* actions per Q row, 1..EVX_LSTATS_MAX_A */
    int32_t pad0;
    /* the probe in progress */
    uint8_t *open;         /* 1 while the env's episode has a probe */
    double *q0;            /* the act's value at the episode's first step */
    double *g;             /* the discounted return so far */
    double *disc;          /* gamma^len */
    int32_t *len;          /* steps so far */
    /* the window: probes folded since the last clear */
    int64_t *w_n;          /* probes with a finite q0 */
    int64_t *w_bad;        /* probes whose q0 was not finite (counted here and nowhere else) */
    double *w_q, *w_g;     /* sums of q0, of g */
    double *w_e, *w_e2;    /* sums of err = q0 - g, of err err */
    double *w_q2, *w_g2, *w_qg; /* sums of q0 q0, g g, q0 g */
    double *w_emin, *w_emax;    /* smallest / largest err (+inf / -inf when empty) */
} evx_vprobe;

/* One row of evx_vprobe_reduce: the window summed over a set of envs. */
typedef struct {
    int64_t probes, bad;
    int64_t open;          /* envs of the row whose probe is in progress */
    double q_sum, g_sum, e_sum, e2_sum, q2_sum, g2_sum, qg_sum, e_min, e_max;
} evx_vprobe_row;

/* No probe in progress, empty window (one launch). */
int evx_vprobe_init(const evx_vprobe *vp, void *stream);
/* One step of every env of vp, one launch, one thread per env. Q [E R][A] f32 and act [E R] are
 * those of the step whose reward [E] f64 and done [E] are passed (the act's Q of the observation the
 * action was chosen from). Per env e, all f64 and not contracted:
 *   if !open[e]:  s = 0.0; for r = 0..R-1: s = s + (double)Q[e R + r][clamp(act[e R + r], 0, A - 1)]
 *                 q0 = s / R;  g = 0;  disc = 1;  len = 0;  open = 1
 *   g = g + disc * reward[e];  disc = disc * gamma;  len += 1
 *   if done[e]:   !isfinite(q0): w_bad += 1
 *                 else: err = q0 - g; w_n += 1; w_q += q0; w_g += g; w_e += err; w_e2 += err * err;
 *                       w_q2 += q0 * q0; w_g2 += g * g; w_qg += q0 * g; w_emin, w_emax take err
 *                 open = 0
 * -22 with a message, before any launch: a NULL descriptor, descriptor array, Q, act, reward or done;
 * E, R or A < 1; A > EVX_LSTATS_MAX_A; gamma not finite or outside [0, 1]. */
int evx_vprobe_update(const evx_vprobe *vp, const float *Q, const int32_t *act, const double *reward,
                      const uint8_t *done, double gamma, void *stream);
/* Closes the probes of the envs with mask[e] != 0 (NULL: all) without folding them: for envs reset
 * from outside the step. */
int evx_vprobe_discard(const evx_vprobe *vp, const uint8_t *mask, void *stream);
/* The window summed over envs into out[0 .. n_layouts] (rows as in evx_episode_reduce) in
 * evx_episode_reduce's fixed order: thread t of EVX_EPISODE_REDUCE_SPAN adds the row's envs t,
 * t + SPAN, ... ascending onto 0.0 (envs of other layouts are skipped), then the thread sums are added
 * pairwise, s[t] = s[t] + s[t + h] for h = SPAN/2, ..., 1. Integer fields are exact. clear != 0: the
 * window arrays are emptied by a second launch; the probes in progress stay. */
int evx_vprobe_reduce(const evx_vprobe *vp, const int32_t *layout_idx, int32_t n_layouts, evx_vprobe_row *out,
                      int32_t clear, void *stream);

#ifdef __cplusplus
}
#endif
#endif
