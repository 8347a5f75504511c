// MI355X (gfx950) terminal health of the vectorised envs, kept on the device.
//
// The reference's strategy comparison (runners/evaluate_strategies.py) prints each episode's
// EvacuationEnv.get_performance_metrics() (envs/evacuation_env.py:290-309): avg_health =
// np.mean of the healths of the persons that are not dead, min_health = their min (100 when there
// are none). With resets fused into the step launch a finished env's persons are gone one launch
// later, so the same numbers are taken here, from pk / health as the step left them and before
// any reset, one wave per env; envs that did not finish leave at once.
//
// avg_health carries numpy's summation order (below) so that it equals np.mean bit for bit.
// Everything else is per env, as in episode.hip: no float atomics, and the only sums over envs
// are in the reduce, in evx_episode_reduce's fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "evacx.h"
#include "evx_device.h"
#include "evx_host.h"
#include "evx_reduce.h"

namespace evxhl {

constexpr int NT = 256;                      // init / clear: one env per thread
constexpr int WAVE = 64;                     // update: one wave per env
constexpr int LEAF_CAP = 256;                // numpy pairwise leaves of one chunk (a leaf of a split holds > 56
                                             // elements, so a chunk of <= 8192 has < 147 of them)
constexpr int NP_CHUNK = 8192;               // np.mean's reduction buffer: elements per pairwise sum
constexpr uint32_t DEAD_BIT = 1u << 25;      // pk: the person is dead
using evxr::RT, evxr::in_row, evxr::tree, evxr::AddI, evxr::AddD, evxr::MinD;

// np.mean of `n` compacted healths in `a` (LDS), the whole wave; the result is valid on lane 0.
// numpy cuts the list into consecutive chunks of NP_CHUNK elements, sums each chunk with its
// pairwise sum (DOUBLE_pairwise_sum) and adds the chunk sums left to right onto the first.
// A chunk's leaves (<= 128 elements) are summed eight at a time: lane = 8 * slot + k carries
// numpy's strided accumulator r[k] of leaf `slot`; the accumulators meet as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) through three shuffles, the tail is added in order by k = 0.
__device__ __forceinline__ double np_mean_sum(const double* a, int n, int* ltab, double* leafsum, int* stk,
                                              double* left, int* nleaf_s) {
    const int lane = threadIdx.x;
    const int slot = lane >> 3, k = lane & 7;
    double total = 0.0;
    for (int c0 = 0; c0 < n; c0 += NP_CHUNK) {
        const int nc = n - c0 < NP_CHUNK ? n - c0 : NP_CHUNK;
        if (lane == 0) *nleaf_s = evx::np_pairwise_leaves(nc, ltab, ltab + LEAF_CAP, LEAF_CAP, stk);
        __syncthreads();
        const int nleaf = *nleaf_s;  // < LEAF_CAP for nc <= NP_CHUNK
        for (int l0 = 0; l0 < nleaf; l0 += 8) {
            const int li = l0 + slot;
            const bool on = li < nleaf;
            const int len = on ? ltab[LEAF_CAP + li] : 0;
            const double* p = a + c0 + (on ? ltab[li] : 0);
            const int body = len - (len % 8);
            double r = 0.0;
            if (len >= 8) {
                r = p[k];
                for (int i = 8; i < body; i += 8) r = r + p[i + k];
            }
            // every lane takes the shuffles; k = 0 holds numpy's combine
            r = r + __shfl_down(r, 1, WAVE);
            r = r + __shfl_down(r, 2, WAVE);
            r = r + __shfl_down(r, 4, WAVE);
            if (on && k == 0) {
                double res = r;
                int i = body;
                if (len < 8) {  // numpy's plain loop
                    res = 0.0;
                    i = 0;
                }
                for (; i < len; i++) res = res + p[i];
                leafsum[li] = res;
            }
        }
        __syncthreads();
        if (lane == 0) {
            const double s = evx::np_pairwise_combine(nc, leafsum, stk, left);
            total = c0 == 0 ? s : total + s;
        }
        __syncthreads();
    }
    return total;
}

// One wave per env. The not-dead healths are compacted in person order into LDS (ballot + prefix
// popcount), summed in numpy's order and folded into the env's slots by lane 0.
__global__ __launch_bounds__(WAVE) void health_update_kernel(evx_health h, const uint32_t* __restrict__ pk,
                                                             const double* __restrict__ health, int P,
                                                             const uint8_t* __restrict__ done, int64_t cap) {
    extern __shared__ __attribute__((aligned(16))) double vals[];  // [P]
    __shared__ int ltab[2 * LEAF_CAP];
    __shared__ double leafsum[LEAF_CAP];
    __shared__ int stk[64];
    __shared__ double left[32];
    __shared__ int nleaf_s;
    const int e = blockIdx.x, lane = threadIdx.x;
    if (!done[e]) return;
    const uint32_t* pke = pk + (int64_t)e * P;
    const double* he = health + (int64_t)e * P;
    int n = 0;
    double mn = INFINITY;
    for (int base = 0; base < P; base += WAVE) {
        const int i = base + lane;
        const bool live = i < P && !(pke[i] & DEAD_BIT);
        const uint64_t m = __ballot(live);
        if (live) {
            const double v = he[i];
            vals[n + __popcll(m & ((1ull << lane) - 1ull))] = v;
            mn = v < mn ? v : mn;
        }
        n += __popcll(m);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(mn, d, WAVE);
        mn = o < mn ? o : mn;
    }
    __syncthreads();
    const double total = np_mean_sum(vals, n, ltab, leafsum, stk, left, &nleaf_s);
    if (lane != 0) return;
    const double avg = n > 0 ? total / (double)n : NAN;  // np.mean([]) is nan
    const double lo = n > 0 ? mn : 100.0;                // min(..., default=100)
    const int64_t k = h.n_total[e];                      // this episode's lifetime index
    if (cap <= 0 || k < cap) {
        h.w_n[e] += 1;
        h.w_alive[e] += n;
        if (n > 0) {
            h.w_has[e] += 1;
            h.w_avg[e] = h.w_avg[e] + avg;
        }
        h.w_min[e] = h.w_min[e] + lo;
        if (lo < h.w_lo[e]) h.w_lo[e] = lo;
    }
    h.last_avg[e] = avg;
    h.last_min[e] = lo;
    h.last_alive[e] = n;
    if (h.tab_slots > 0 && k < h.tab_slots) {
        const int64_t j = (int64_t)e * h.tab_slots + k;
        h.tab_avg[j] = avg;
        h.tab_min[j] = lo;
        h.tab_alive[j] = n;
    }
    h.n_total[e] = k + 1;
}

__global__ __launch_bounds__(NT) void health_clear_kernel(evx_health h, int all) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= h.E) return;
    h.w_n[e] = 0;
    h.w_has[e] = 0;
    h.w_alive[e] = 0;
    h.w_avg[e] = 0.0;
    h.w_min[e] = 0.0;
    h.w_lo[e] = INFINITY;
    if (all) {
        h.last_avg[e] = 0.0;
        h.last_min[e] = 0.0;
        h.last_alive[e] = 0;
        h.n_total[e] = 0;
    }
}

// One workgroup per output row, in the order of evx_reduce.h.
__global__ __launch_bounds__(RT) void health_reduce_kernel(evx_health h, const int32_t* __restrict__ layout_idx,
                                                           int n_layouts, evx_health_row* __restrict__ out) {
    __shared__ double shd[RT];
    __shared__ int64_t shi[RT];
    const int row = blockIdx.x, t = threadIdx.x;
    int64_t n = 0, has = 0, alive = 0;
    double avg = 0.0, mins = 0.0, lo = INFINITY;
    for (int e = t; e < h.E; e += RT) {
        if (!in_row(layout_idx, n_layouts, row, e)) continue;
        n += h.w_n[e];
        has += h.w_has[e];
        alive += h.w_alive[e];
        avg = avg + h.w_avg[e];
        mins = mins + h.w_min[e];
        const double l = h.w_lo[e];
        lo = l < lo ? l : lo;
    }
    evx_health_row o;
    o.episodes = tree(shi, t, n, AddI());
    o.health_episodes = tree(shi, t, has, AddI());
    o.alive_sum = tree(shi, t, alive, AddI());
    o.avg_sum = tree(shd, t, avg, AddD());
    o.min_sum = tree(shd, t, mins, AddD());
    o.min_min = tree(shd, t, lo, MinD());
    if (t == 0) out[row] = o;
}

}  // namespace evxhl

namespace {
using evxh::blocks;
using evxh::fail;
using evxh::failf;
using evxh::hip_status;
int check_h(const evx_health* h, const char* who) {
    if (!h) return failf(-22, "%s: NULL health descriptor", who);
    if (h->E < 1) return failf(-22, "%s: E must be >= 1", who);
    if (!h->n_total || !h->w_n || !h->w_has || !h->w_alive || !h->w_avg || !h->w_min || !h->w_lo || !h->last_avg ||
        !h->last_min || !h->last_alive)
        return failf(-22, "%s: NULL health buffer", who);
    if (h->tab_slots < 0 || (h->tab_slots > 0 && (!h->tab_avg || !h->tab_min || !h->tab_alive)))
        return failf(-22, "%s: health table slots without its buffers", who);
    return 0;
}
}  // namespace

extern "C" {

const char* evx_health_last_error(void) { return evxh::g_err; }

int evx_health_init(const evx_health* h, void* stream) {
    if (int rc = check_h(h, "health_init")) return rc;
    hipLaunchKernelGGL(evxhl::health_clear_kernel, dim3(blocks(h->E, evxhl::NT)), dim3(evxhl::NT), 0,
                       (hipStream_t)stream, *h, 1);
    return hip_status("health_init");
}

int evx_health_update(const evx_health* h, const int32_t* pk, const double* health, int32_t P, const uint8_t* done,
                      int64_t cap, void* stream) {
    if (int rc = check_h(h, "health_update")) return rc;
    if (!pk || !health || !done) return fail(-22, "health_update: NULL pk, health or done");
    if (P < 1 || P > EVX_HEALTH_MAX_P) return fail(-22, "health_update: P must be 1..16383");
    const size_t lds = (size_t)P * sizeof(double);  // the compacted healths
    hipLaunchKernelGGL(evxhl::health_update_kernel, dim3((unsigned)h->E), dim3(evxhl::WAVE), lds, (hipStream_t)stream,
                       *h, (const uint32_t*)pk, health, (int)P, done, cap);
    return hip_status("health_update");
}

int evx_health_reduce(const evx_health* h, const int32_t* layout_idx, int32_t n_layouts, evx_health_row* out,
                      int32_t clear, void* stream) {
    if (int rc = check_h(h, "health_reduce")) return rc;
    if (int rc = evxr::check_rows("health_reduce", out, n_layouts, layout_idx)) return rc;
    return evxr::reduce_rows("health_reduce", stream, clear, evxhl::health_reduce_kernel, evxhl::health_clear_kernel,
                             evxhl::NT, *h, layout_idx, n_layouts, out);
}

}  // extern "C"
