// MI355X (gfx950) evacuation timelines and tracked persons of the vectorised envs, kept on the device.
//
// The reference judges a trained policy with one recorded episode (DQNTrainingVisualizer,
// utils/visualization.py): evacuated / dead / remaining / avg_health after every step, the
// evacuation-time and death-time distributions from the per-step count deltas, and the positions
// and health of some selected persons. Here the same is taken from every env's step outputs
// (counts, done) and, with resets apart, from pk / health as the step left them: per layout row
// and episode step, the events and the health of every episode that is recorded are added up.
//
// Every accumulator that is added across envs is an integer -- counts, and health in fixed point
// at 2^-20 -- so the order of the adds cannot change a bit; there are no float atomics. A
// workgroup first combines its envs that fall on the same (row, slot) in LDS, then issues one
// returnless 64-bit atomic add per field and distinct destination.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "evacx.h"
#include "evx_host.h"

namespace evxt {

constexpr int NT = 256;                  // init, trace: one element / tracked person per thread
constexpr int WAVE = 64;                 // update: one wave per env
constexpr int WPB = 8;                   // update: envs (waves) per workgroup
constexpr int NF = 6;                    // fields of a slot: evac, dead, ended, seen, alive, health_q
constexpr uint32_t DEAD_BIT = 1u << 25;  // pk: the person is dead
constexpr double Q_ONE = 1048576.0;      // 2^20: health_q's unit is 2^-20
constexpr double H_MAX = 128.0;          // |health| beyond this is counted in bad_health, not summed

__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
    if (v != 0) (void)atomicAdd((unsigned long long*)p, (unsigned long long)v);  // result unused: returnless
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One thread per tracked person: its pk / health after the step that is about to be counted go to
// trace slot t[e] + 1 (slot0: after the reset, to slot 0), while its env's first episode runs. t
// and n_total are read here, before the update launch of the same call bumps them (stream order).
__global__ __launch_bounds__(NT) void timeline_trace_kernel(evx_timeline tl, const uint32_t* __restrict__ pk,
                                                            const double* __restrict__ health, int P, int slot0) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= tl.n_trk) return;
    const int e = clampi(tl.trk_env[i], tl.E - 1), p = clampi(tl.trk_person[i], P - 1);
    if (tl.n_total[e] != 0) return;
    const int64_t slot = slot0 ? 0 : (int64_t)tl.t[e] + 1;
    if (slot < 0 || slot > tl.T) return;
    const int64_t j = slot * tl.n_trk + i, src = (int64_t)e * P + p;
    tl.trk_pk[j] = pk[src];
    tl.trk_health[j] = health[src];
    tl.trk_len[i] = (int32_t)slot + 1;
}

// One wave per env, WPB envs per workgroup. The wave scans its env's persons in 64-person passes
// (ballot + popcount for alive, one i64 accumulator per lane for health_q, an integer butterfly);
// lane 0 forms the count deltas and advances the env's episode; then the workgroup's envs that fall
// on the same (row, slot) are added in LDS and the first of them goes to memory.
__global__ __launch_bounds__(WPB* WAVE) void timeline_update_kernel(evx_timeline tl, const int32_t* __restrict__ counts,
                                                                    const uint8_t* __restrict__ done,
                                                                    const int32_t* __restrict__ layout_idx,
                                                                    const uint32_t* __restrict__ pk,
                                                                    const double* __restrict__ health, int P,
                                                                    int64_t cap) {
    __shared__ int64_t s_key[WPB];      // row * (T + 1) + min(slot, T); -1: nothing to add
    __shared__ int64_t s_val[WPB][NF];
    const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int e = blockIdx.x * WPB + w;
    int64_t key = -1;
    int64_t v[NF] = {0, 0, 0, 0, 0, 0};
    if (e < tl.E) {
        const int32_t t = tl.t[e];
        const int64_t k = tl.n_total[e];  // this episode's lifetime index
        const bool in = cap <= 0 || k < cap;
        const bool slotted = t >= 0 && t < tl.T;
        int64_t q = 0;
        int n_alive = 0, n_bad = 0;
        if (pk && in && slotted) {
            const uint32_t* pke = pk + (int64_t)e * P;
            const double* he = health + (int64_t)e * P;
            for (int base = 0; base < P; base += WAVE) {
                const int i = base + lane;
                const bool live = i < P && !(pke[i] & DEAD_BIT);
                const double h = live ? he[i] : 0.0;
                const bool ok = live && fabs(h) <= H_MAX;  // a NaN is not ok
                n_alive += __popcll(__ballot(ok));
                n_bad += __popcll(__ballot(live && !ok));
                if (ok) q += llrint(h * Q_ONE);  // exact product, round half even
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor((long long)q, d, WAVE);
        }
        if (lane == 0) {
            const int32_t ev = counts[2 * e], dd = counts[2 * e + 1];
            const bool fin = done[e] != 0;
            if (in) {
                const int row = layout_idx ? clampi(layout_idx[e], tl.n_rows - 1) : 0;
                key = (int64_t)row * ((int64_t)tl.T + 1) + (slotted ? t : tl.T);
                v[0] = (int64_t)ev - tl.p_evac[e];
                v[1] = (int64_t)dd - tl.p_dead[e];
                v[2] = fin ? 1 : 0;
                v[3] = 1;
                v[4] = n_alive;
                v[5] = q;
                if (n_bad) add64(tl.bad_health, n_bad);
            }
            if (fin) {
                tl.t[e] = 0;
                tl.p_evac[e] = 0;
                tl.p_dead[e] = 0;
                tl.n_total[e] = k + 1;
            } else {
                tl.t[e] = t < INT32_MAX ? t + 1 : t;
                tl.p_evac[e] = ev;
                tl.p_dead[e] = dd;
            }
        }
    }
    if (lane == 0) {
        s_key[w] = key;
#pragma unroll
        for (int f = 0; f < NF; f++) s_val[w][f] = v[f];
    }
    __syncthreads();
    if (lane != 0 || key < 0) return;
    for (int u = 0; u < w; u++)
        if (s_key[u] == key) return;  // an earlier wave of the workgroup carries this destination
    for (int u = w + 1; u < WPB; u++)
        if (s_key[u] == key) {
#pragma unroll
            for (int f = 0; f < NF; f++) v[f] += s_val[u][f];
        }
    const int64_t row = key / ((int64_t)tl.T + 1), slot = key % ((int64_t)tl.T + 1);
    if (slot < tl.T) {
        const int64_t j = row * tl.T + slot;
        add64(tl.evac + j, v[0]);
        add64(tl.dead + j, v[1]);
        add64(tl.ended + j, v[2]);
        add64(tl.seen + j, v[3]);
        add64(tl.alive + j, v[4]);
        add64(tl.health_q + j, v[5]);
    } else {  // beyond the table: counted, never dropped
        int64_t* l = tl.late + row * 4;
        add64(l + 0, v[0]);
        add64(l + 1, v[1]);
        add64(l + 2, v[2]);
        add64(l + 3, v[3]);
    }
}

// Everything the timeline writes is zeroed (trk_env / trk_person are the caller's input).
__global__ __launch_bounds__(NT) void timeline_init_kernel(evx_timeline tl) {
    const int64_t slots = (int64_t)tl.n_rows * tl.T, trace = ((int64_t)tl.T + 1) * tl.n_trk;
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < slots; i += stride) {
        tl.evac[i] = 0;
        tl.dead[i] = 0;
        tl.ended[i] = 0;
        tl.seen[i] = 0;
        tl.alive[i] = 0;
        tl.health_q[i] = 0;
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < tl.E; i += stride) {
        tl.t[i] = 0;
        tl.p_evac[i] = 0;
        tl.p_dead[i] = 0;
        tl.n_total[i] = 0;
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < (int64_t)tl.n_rows * 4; i += stride) tl.late[i] = 0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < trace; i += stride) {
        tl.trk_pk[i] = 0;
        tl.trk_health[i] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < tl.n_trk; i += stride) tl.trk_len[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) tl.bad_health[0] = 0;
}

}  // namespace evxt

namespace {
using evxh::blocks;
using evxh::fail;
using evxh::failf;
using evxh::hip_status;
int check_tl(const evx_timeline* tl, const char* who) {
    const char* what = nullptr;
    if (!tl)
        what = "NULL timeline descriptor";
    else if (tl->E < 1 || tl->T < 1)
        what = "E and T must be >= 1";
    else if (tl->n_rows < 1)
        what = "n_rows must be >= 1";
    else if (!tl->t || !tl->p_evac || !tl->p_dead || !tl->n_total || !tl->evac || !tl->dead || !tl->ended ||
             !tl->seen || !tl->alive || !tl->health_q || !tl->late || !tl->bad_health)
        what = "NULL timeline buffer";
    else if (tl->n_trk < 0)
        what = "n_trk must be >= 0";
    else if (tl->n_trk > 0 && (!tl->trk_env || !tl->trk_person || !tl->trk_pk || !tl->trk_health || !tl->trk_len))
        what = "tracked persons without their trace arrays";
    return what ? failf(-22, "%s: %s", who, what) : 0;
}
}  // namespace

extern "C" {

const char* evx_timeline_last_error(void) { return evxh::g_err; }

int evx_timeline_init(const evx_timeline* tl, void* stream) {
    if (int rc = check_tl(tl, "timeline_init")) return rc;
    int64_t n = (int64_t)tl->n_rows * tl->T;
    const int64_t trace = ((int64_t)tl->T + 1) * tl->n_trk;
    n = n > tl->E ? n : tl->E;
    n = n > trace ? n : trace;
    const unsigned grid = blocks(n, evxt::NT);
    hipLaunchKernelGGL(evxt::timeline_init_kernel, dim3(grid < 4096u ? grid : 4096u), dim3(evxt::NT), 0,
                       (hipStream_t)stream, *tl);
    return hip_status("timeline_init");
}

int evx_timeline_update(const evx_timeline* tl, const int32_t* counts, const uint8_t* done, const int32_t* layout_idx,
                        const int32_t* pk, const double* health, int32_t P, int64_t cap, void* stream) {
    if (int rc = check_tl(tl, "timeline_update")) return rc;
    if (!counts || !done) return fail(-22, "timeline_update: NULL counts or done");
    if (P < 1 || P > EVX_HEALTH_MAX_P) return fail(-22, "timeline_update: P must be 1..16383");
    if ((pk == nullptr) != (health == nullptr)) return fail(-22, "timeline_update: pk and health go together");
    if (tl->n_trk > 0 && !pk) return fail(-22, "timeline_update: tracked persons need pk and health");
    const hipStream_t st = (hipStream_t)stream;
    if (tl->n_trk > 0) {  // first: it reads t and n_total as they are before this step is counted
        hipLaunchKernelGGL(evxt::timeline_trace_kernel, dim3(blocks(tl->n_trk, evxt::NT)), dim3(evxt::NT), 0, st, *tl,
                           (const uint32_t*)pk, health, (int)P, 0);
        if (int rc = hip_status("timeline_update (trace)")) return rc;
    }
    hipLaunchKernelGGL(evxt::timeline_update_kernel, dim3(blocks(tl->E, evxt::WPB)), dim3(evxt::WPB * evxt::WAVE), 0,
                       st, *tl, counts, done, layout_idx, (const uint32_t*)pk, health, (int)P, cap);
    return hip_status("timeline_update");
}

int evx_timeline_trace0(const evx_timeline* tl, const int32_t* pk, const double* health, int32_t P, void* stream) {
    if (int rc = check_tl(tl, "timeline_trace0")) return rc;
    if (!pk || !health) return fail(-22, "timeline_trace0: NULL pk or health");
    if (P < 1 || P > EVX_HEALTH_MAX_P) return fail(-22, "timeline_trace0: P must be 1..16383");
    if (tl->n_trk == 0) return 0;
    hipLaunchKernelGGL(evxt::timeline_trace_kernel, dim3(blocks(tl->n_trk, evxt::NT)), dim3(evxt::NT), 0,
                       (hipStream_t)stream, *tl, (const uint32_t*)pk, health, (int)P, 1);
    return hip_status("timeline_trace0");
}

}  // extern "C"
