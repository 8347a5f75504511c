// MI355X (gfx950) spatial maps of the vectorised envs, kept on the device: per layout row and grid
// cell, the persons that arrived, stood still, left through an exit or died there, and the robots'
// positions, over every counted episode of every env (include/evacx.h, evx_spatial_*).
//
// The update compares every person's pk with the env's previous one (prev). The two dense maps,
// arrive and stall, take one add per live person and step: they are counted in LDS as u32 and
// flushed once per workgroup and row with returnless 64-bit atomics. A workgroup folds at most
// EPW_MAX envs of at most EVX_HEALTH_MAX_P persons between two flushes, so a counter cannot
// overflow whatever pk holds. evac, died and robot are sparse and go straight to 64-bit atomics.
// A grid whose two maps do not fit the LDS is cut into x-bands, one workgroup column per band;
// prev and n_total are then written by a second launch, after every band has read them.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "evacx.h"
#include "evx_host.h"

namespace evxs {

constexpr int NT = 1024;                 // update: 16 waves, one env per wave at a time
constexpr int NT_FLAT = 256;             // init: one element per thread
constexpr int WAVE = 64;
constexpr int NW = NT / WAVE;
constexpr int UNR = 4;                   // 64-person passes in flight per wave
constexpr int LDS_MAX = 160 * 1024;
constexpr int LDS_HDR = 64;              // bytes in front of the counters: the row scan's word
constexpr int CELLS_MAX = (LDS_MAX - LDS_HDR) / 8;  // cells of one band: two u32 counters each
constexpr int EPW_MIN = NW, EPW_MAX = 1024;  // EPW_MAX * EVX_HEALTH_MAX_P < 2^32
constexpr int FILL = 16;                 // person adds a workgroup aims at per LDS counter pair
constexpr int GRID_MAX = 4096;           // GX, GY
constexpr uint32_t SAFE_BIT = 1u << 24, DEAD_BIT = 1u << 25, GONE = SAFE_BIT | DEAD_BIT;
static_assert((int64_t)EPW_MAX * EVX_HEALTH_MAX_P < (int64_t)UINT32_MAX, "an LDS counter must hold a whole share");
static_assert(CELLS_MAX >= GRID_MAX, "one column must fit a band");

__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
    (void)atomicAdd((unsigned long long*)p, (unsigned long long)v);  // result unused: returnless
}

__device__ __forceinline__ int row_of(const int32_t* __restrict__ layout_idx, int e, int n_rows) {
    if (!layout_idx) return 0;
    const int r = layout_idx[e];
    return r < 0 ? 0 : (r > n_rows - 1 ? n_rows - 1 : r);
}

// Workgroup (s, b): envs [s * epw, (s + 1) * epw) and the columns [b * bw, (b + 1) * bw). The rows
// the share holds are taken in ascending order (a block-wide minimum finds the next); for one row,
// each wave folds the share's envs of that row one at a time, then the workgroup flushes and
// clears its counters. FUSED (one band): the wave also writes prev and bumps n_total.
template <bool FUSED>
__global__ __launch_bounds__(NT) void spatial_update_kernel(evx_spatial sp, const uint32_t* __restrict__ pk,
                                                            const uint32_t* __restrict__ robots,
                                                            const uint8_t* __restrict__ done,
                                                            const int32_t* __restrict__ layout_idx, int64_t cap,
                                                            int epw, int bw) {
    extern __shared__ uint32_t lds[];
    int* s_next = (int*)lds;
    uint32_t* h = lds + LDS_HDR / 4;  // arrive [gb], stall [gb]
    const int tid = threadIdx.x, w = tid / WAVE, lane = tid % WAVE;
    const int GX = sp.GX, GY = sp.GY, P = sp.P, R = sp.R;
    const int64_t G = (int64_t)GX * GY;
    const int band = blockIdx.y;
    const int x0 = band * bw, x1 = x0 + bw < GX ? x0 + bw : GX;
    const int gb = (x1 - x0) * GY;
    const int64_t e0 = (int64_t)blockIdx.x * epw;
    const int e1 = (int)(e0 + epw < sp.E ? e0 + epw : sp.E);
    for (int i = tid; i < 2 * gb; i += NT) h[i] = 0;
    int last = -1;
    for (;;) {
        if (tid == 0) *s_next = INT_MAX;
        __syncthreads();  // also: the counters are clear
        for (int e = (int)e0 + tid; e < e1; e += NT) {
            const int r = row_of(layout_idx, e, sp.n_rows);
            if (r > last) atomicMin(s_next, r);
        }
        __syncthreads();
        const int row = *s_next;
        if (row == INT_MAX) break;
        last = row;
        int64_t* const evac = sp.evac + row * G;
        int64_t* const died = sp.died + row * G;
        int n_steps = 0, n_bad = 0;
        for (int e = (int)e0 + w; e < e1; e += NW) {
            if (row_of(layout_idx, e, sp.n_rows) != row) continue;
            const int64_t k = sp.n_total[e];
            const bool counted = cap <= 0 || k < cap;
            uint32_t* const pe = sp.prev + (int64_t)e * P;
            const uint32_t* const ce = pk + (int64_t)e * P;
            for (int base = 0; base < P; base += WAVE * UNR) {
                uint32_t old[UNR], cur[UNR];
#pragma unroll
                for (int u = 0; u < UNR; u++) {
                    const int i = base + u * WAVE + lane;
                    old[u] = i < P ? pe[i] : GONE;
                    cur[u] = i < P ? ce[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < UNR; u++) {
                    const int i = base + u * WAVE + lane;
                    const uint32_t o = old[u], c = cur[u];
                    if (FUSED && i < P && o != c) pe[i] = c;
                    if (!counted || (o & GONE)) continue;
                    const int x = c & 0xfff, y = (c >> 12) & 0xfff;
                    if (x >= GX || y >= GY) {
                        n_bad += band == 0;
                        continue;
                    }
                    if (x < x0 || x >= x1) continue;
                    const int cell = x * GY + y, lc = cell - x0 * GY;
                    if (c & SAFE_BIT) {
                        add64(evac + cell, 1);
                    } else if (c & DEAD_BIT) {
                        add64(died + cell, 1);
                    } else {
                        const int ocell = (int)(o & 0xfff) * GY + (int)((o >> 12) & 0xfff);
                        atomicAdd(&h[cell != ocell ? lc : gb + lc], 1u);  // result unused
                    }
                }
            }
            if (counted && band == 0) {
                for (int r = lane; r < R; r += WAVE) {
                    const uint32_t v = robots[(int64_t)e * R + r];
                    const int x = v & 0xffff, y = v >> 16;
                    if (x >= GX || y >= GY)
                        n_bad++;
                    else
                        add64(sp.robot + row * G + (x * GY + y), 1);
                }
                n_steps++;
            }
            if (FUSED && lane == 0 && done[e]) sp.n_total[e] = k + 1;
        }
        if (band == 0) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) n_bad += __shfl_xor(n_bad, d, WAVE);
            if (lane == 0 && n_bad) add64(sp.bad, n_bad);
            if (lane == 0 && n_steps) add64(sp.steps + row, n_steps);
        }
        __syncthreads();
        int64_t* const arrive = sp.arrive + row * G + (int64_t)x0 * GY;
        int64_t* const stall = sp.stall + row * G + (int64_t)x0 * GY;
        for (int i = tid; i < gb; i += NT) {
            const uint32_t a = h[i], s = h[gb + i];
            if (a) {
                add64(arrive + i, a);
                h[i] = 0;
            }
            if (s) {
                add64(stall + i, s);
                h[gb + i] = 0;
            }
        }
    }
}

// One wave per env: prev[e] = pk[e] where mask[e] (NULL: every env), and with done the step is
// taken as well (n_total). evx_spatial_sync, and the second launch of the banded update.
__global__ __launch_bounds__(NT) void spatial_copy_kernel(evx_spatial sp, const uint32_t* __restrict__ pk,
                                                          const uint8_t* __restrict__ mask,
                                                          const uint8_t* __restrict__ done) {
    const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t e = (int64_t)blockIdx.x * NW + w;
    if (e >= sp.E) return;
    if (!mask || mask[e]) {
        uint32_t* const pe = sp.prev + e * sp.P;
        const uint32_t* const ce = pk + e * sp.P;
        for (int i = lane; i < sp.P; i += WAVE) {
            const uint32_t c = ce[i];
            if (pe[i] != c) pe[i] = c;
        }
    }
    if (done && lane == 0 && done[e]) sp.n_total[e] += 1;
}

__global__ __launch_bounds__(NT_FLAT) void spatial_init_kernel(evx_spatial sp) {
    const int64_t cells = (int64_t)sp.n_rows * sp.GX * sp.GY, persons = (int64_t)sp.E * sp.P;
    const int64_t stride = (int64_t)gridDim.x * NT_FLAT, first = (int64_t)blockIdx.x * NT_FLAT + threadIdx.x;
    for (int64_t i = first; i < persons; i += stride) sp.prev[i] = 0;
    for (int64_t i = first; i < cells; i += stride) {
        sp.arrive[i] = 0;
        sp.stall[i] = 0;
        sp.evac[i] = 0;
        sp.died[i] = 0;
        sp.robot[i] = 0;
    }
    for (int64_t i = first; i < sp.E; i += stride) sp.n_total[i] = 0;
    for (int64_t i = first; i < sp.n_rows; i += stride) sp.steps[i] = 0;
    if (first == 0) sp.bad[0] = 0;
}

}  // namespace evxs

namespace {
using evxh::blocks;
using evxh::fail;
using evxh::failf;
using evxh::hip_status;

const char* check_sizes(int32_t GX, int32_t GY, int32_t P, int32_t n_rows) {
    if (P < 1 || P > EVX_HEALTH_MAX_P) return "P must be 1..16383";
    if (GX < 1 || GY < 1 || GX > evxs::GRID_MAX || GY > evxs::GRID_MAX) return "GX and GY must be 1..4096";
    if (n_rows < 1) return "n_rows must be >= 1";
    return nullptr;
}

// The one place the route is decided: evx_spatial_update launches what this returns and
// evx_spatial_plan reports it. Sizes are checked by the callers.
evx_spatial_launch make_plan(int32_t GX, int32_t GY, int32_t P) {
    evx_spatial_launch pl;
    const int64_t G = (int64_t)GX * GY;
    if (G <= evxs::CELLS_MAX) {
        pl.route = EVX_SPATIAL_LDS;
        pl.bands = 1;
        pl.band_w = GX;
    } else {
        const int cols = evxs::CELLS_MAX / GY;  // >= 4: GY <= 4096
        pl.route = EVX_SPATIAL_BANDS;
        pl.bands = (GX + cols - 1) / cols;
        pl.band_w = (GX + pl.bands - 1) / pl.bands;  // even bands, each <= cols wide
    }
    pl.band_cells = pl.band_w * GY;
    pl.lds_bytes = evxs::LDS_HDR + 8 * pl.band_cells;
    int64_t epw = ((int64_t)evxs::FILL * pl.band_cells + P - 1) / P;
    epw = (epw + evxs::NW - 1) / evxs::NW * evxs::NW;
    pl.envs_per_wg = (int32_t)(epw < evxs::EPW_MIN ? evxs::EPW_MIN : (epw > evxs::EPW_MAX ? evxs::EPW_MAX : epw));
    pl.threads = evxs::NT;
    pl.launches = pl.bands > 1 ? 2 : 1;
    return pl;
}

int check_sp(const evx_spatial* sp, const char* who) {
    const char* what = nullptr;
    if (!sp)
        what = "NULL spatial descriptor";
    else if (sp->E < 1)
        what = "E must be >= 1";
    else if (sp->R < 0)
        what = "R must be >= 0";
    else if (const char* s = check_sizes(sp->GX, sp->GY, sp->P, sp->n_rows))
        what = s;
    else if (!sp->prev || !sp->n_total || !sp->arrive || !sp->stall || !sp->evac || !sp->died || !sp->robot ||
             !sp->steps || !sp->bad)
        what = "NULL spatial buffer";
    return what ? failf(-22, "%s: %s", who, what) : 0;
}
}  // namespace

extern "C" {

const char* evx_spatial_last_error(void) { return evxh::g_err; }

int evx_spatial_plan(int32_t GX, int32_t GY, int32_t P, int32_t n_rows, evx_spatial_launch* plan) {
    if (!plan) return fail(-22, "spatial_plan: NULL plan");
    if (const char* s = check_sizes(GX, GY, P, n_rows)) return failf(-22, "spatial_plan: %s", s);
    *plan = make_plan(GX, GY, P);
    return 0;
}

int evx_spatial_init(const evx_spatial* sp, void* stream) {
    if (int rc = check_sp(sp, "spatial_init")) return rc;
    int64_t n = (int64_t)sp->E * sp->P;
    const int64_t cells = (int64_t)sp->n_rows * sp->GX * sp->GY;
    n = n > cells ? n : cells;
    const unsigned grid = blocks(n, evxs::NT_FLAT);
    hipLaunchKernelGGL(evxs::spatial_init_kernel, dim3(grid < 4096u ? grid : 4096u), dim3(evxs::NT_FLAT), 0,
                       (hipStream_t)stream, *sp);
    return hip_status("spatial_init");
}

int evx_spatial_sync(const evx_spatial* sp, const int32_t* pk, const uint8_t* mask, void* stream) {
    if (int rc = check_sp(sp, "spatial_sync")) return rc;
    if (!pk) return fail(-22, "spatial_sync: NULL pk");
    hipLaunchKernelGGL(evxs::spatial_copy_kernel, dim3(blocks(sp->E, evxs::NW)), dim3(evxs::NT), 0, (hipStream_t)stream,
                       *sp, (const uint32_t*)pk, mask, (const uint8_t*)nullptr);
    return hip_status("spatial_sync");
}

int evx_spatial_update(const evx_spatial* sp, const int32_t* pk, const int32_t* robots, const uint8_t* done,
                       const int32_t* layout_idx, int64_t cap, void* stream) {
    if (int rc = check_sp(sp, "spatial_update")) return rc;
    if (!pk || !done) return fail(-22, "spatial_update: NULL pk or done");
    if (sp->R > 0 && !robots) return fail(-22, "spatial_update: NULL robots with R > 0");
    const evx_spatial_launch pl = make_plan(sp->GX, sp->GY, sp->P);
    static std::atomic<uint64_t> attr_done{0};
    static const void* const ks[] = {(const void*)evxs::spatial_update_kernel<true>,
                                     (const void*)evxs::spatial_update_kernel<false>};
    evxh::max_lds_once(attr_done, ks, 2, evxs::LDS_MAX);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks(sp->E, pl.envs_per_wg), (unsigned)pl.bands);
    if (pl.bands == 1) {
        hipLaunchKernelGGL(evxs::spatial_update_kernel<true>, grid, dim3(evxs::NT), (size_t)pl.lds_bytes, st, *sp,
                           (const uint32_t*)pk, (const uint32_t*)robots, done, layout_idx, cap, pl.envs_per_wg,
                           pl.band_w);
        return hip_status("spatial_update");
    }
    hipLaunchKernelGGL(evxs::spatial_update_kernel<false>, grid, dim3(evxs::NT), (size_t)pl.lds_bytes, st, *sp,
                       (const uint32_t*)pk, (const uint32_t*)robots, done, layout_idx, cap, pl.envs_per_wg, pl.band_w);
    if (int rc = hip_status("spatial_update (bands)")) return rc;
    hipLaunchKernelGGL(evxs::spatial_copy_kernel, dim3(blocks(sp->E, evxs::NW)), dim3(evxs::NT), 0, st, *sp,
                       (const uint32_t*)pk, (const uint8_t*)nullptr, done);
    return hip_status("spatial_update (step)");
}

}  // extern "C"
