// MI355X (gfx950) episode statistics: returns, lengths and outcome counts of the vectorised
// envs, kept on the device.
//
// The reference's training loop (runners/train_dqn.py:129-161) adds every step's reward into
// total_reward on the host and logs the episode when done comes back. The vectorised trainer
// resets finished envs inside the step launch and never sees an episode boundary on the
// host, so the same bookkeeping runs here, one thread per env, from the step's outputs
// (reward, done, counts) before the next step overwrites them.
//
// Everything is per env: an env's numbers are a pure function of that env's own step
// sequence, whatever the order envs, groups or streams run in, and no float atomics are
// needed. The only sums over envs are in the reduce, which adds in one fixed order (below).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "evacx.h"
#include "evx_host.h"
#include "evx_reduce.h"

namespace evxe {

constexpr int NT = 256;  // update / discard / clear: one env per thread
using evxr::RT, evxr::in_row, evxr::tree, evxr::AddI, evxr::AddD, evxr::MinD, evxr::MaxD;

// ret += reward, len += 1 (the reference's total_reward += reward, runners/train_dqn.py:109, in
// step order); a finished episode is folded into the window, the last-episode slots and the
// episode table, then the episode in progress starts again from 0
__global__ __launch_bounds__(NT) void episode_update_kernel(evx_episodes ep, const double* __restrict__ reward,
                                                             const uint8_t* __restrict__ done,
                                                             const int32_t* __restrict__ counts, int64_t cap) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= ep.E) return;
    const double ret = ep.ret[e] + reward[e];
    const int32_t len = ep.len[e] + 1;
    if (!done[e]) {
        ep.ret[e] = ret;
        ep.len[e] = len;
        return;
    }
    const int32_t evac = counts[2 * e], dead = counts[2 * e + 1];
    const int64_t k = ep.n_total[e];  // this episode's lifetime index
    if (cap <= 0 || k < cap) {
        ep.w_n[e] += 1;
        ep.w_len[e] += len;
        ep.w_evac[e] += evac;
        ep.w_dead[e] += dead;
        ep.w_ret[e] += ret;
        ep.w_ret2[e] += ret * ret;
        if (ret < ep.w_min[e]) ep.w_min[e] = ret;
        if (ret > ep.w_max[e]) ep.w_max[e] = ret;
    }
    ep.last_ret[e] = ret;
    ep.last_len[e] = len;
    ep.last_evac[e] = evac;
    ep.last_dead[e] = dead;
    if (ep.tab_slots > 0 && k < ep.tab_slots) {
        const int64_t j = (int64_t)e * ep.tab_slots + k;
        ep.tab_ret[j] = ret;
        ep.tab_len[j] = len;
        ep.tab_evac[j] = evac;
        ep.tab_dead[j] = dead;
    }
    ep.n_total[e] = k + 1;
    ep.ret[e] = 0.0;
    ep.len[e] = 0;
}

__global__ __launch_bounds__(NT) void episode_discard_kernel(evx_episodes ep, const uint8_t* __restrict__ mask) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= ep.E || (mask && !mask[e])) return;
    ep.ret[e] = 0.0;
    ep.len[e] = 0;
}

__device__ __forceinline__ void window_clear(const evx_episodes& ep, int e) {
    ep.w_n[e] = 0;
    ep.w_len[e] = 0;
    ep.w_evac[e] = 0;
    ep.w_dead[e] = 0;
    ep.w_ret[e] = 0.0;
    ep.w_ret2[e] = 0.0;
    ep.w_min[e] = INFINITY;
    ep.w_max[e] = -INFINITY;
}

__global__ __launch_bounds__(NT) void episode_clear_kernel(evx_episodes ep, int all) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= ep.E) return;
    window_clear(ep, e);
    if (all) {
        ep.ret[e] = 0.0;
        ep.len[e] = 0;
        ep.last_ret[e] = 0.0;
        ep.last_len[e] = 0;
        ep.last_evac[e] = 0;
        ep.last_dead[e] = 0;
        ep.n_total[e] = 0;
    }
}

struct Acc {
    int64_t n, len, evac, dead, remaining, none;
    double ret, ret2, mn, mx;
};

__device__ __forceinline__ void acc_add(Acc& a, const Acc& b) {
    a.n += b.n;
    a.len += b.len;
    a.evac += b.evac;
    a.dead += b.dead;
    a.remaining += b.remaining;
    a.none += b.none;
    a.ret = a.ret + b.ret;
    a.ret2 = a.ret2 + b.ret2;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
}

// One workgroup per output row, in the order of evx_reduce.h.
__global__ __launch_bounds__(RT) void episode_reduce_kernel(evx_episodes ep, const int32_t* __restrict__ layout_idx,
                                                            int n_layouts, int64_t cap,
                                                            evx_episode_row* __restrict__ out) {
    __shared__ double shd[RT];
    __shared__ int64_t shi[RT];
    const int row = blockIdx.x, t = threadIdx.x;
    Acc a = {0, 0, 0, 0, 0, 0, 0.0, 0.0, INFINITY, -INFINITY};
    for (int e = t; e < ep.E; e += RT) {
        if (!in_row(layout_idx, n_layouts, row, e)) continue;
        Acc b;
        b.n = ep.w_n[e];
        b.len = ep.w_len[e];
        b.evac = ep.w_evac[e];
        b.dead = ep.w_dead[e];
        const int64_t tot = ep.n_total[e];
        b.remaining = (cap > 0 && tot < cap) ? 1 : 0;
        b.none = tot == 0 ? 1 : 0;
        b.ret = ep.w_ret[e];
        b.ret2 = ep.w_ret2[e];
        b.mn = ep.w_min[e];
        b.mx = ep.w_max[e];
        acc_add(a, b);
    }
    // one field at a time through 8 KB of LDS (the whole Acc of 1024 threads would not fit the
    // 64 KB of static LDS); every field takes the same pairwise tree
    evx_episode_row o;
    o.episodes = tree(shi, t, a.n, AddI());
    o.len_sum = tree(shi, t, a.len, AddI());
    o.evac_sum = tree(shi, t, a.evac, AddI());
    o.dead_sum = tree(shi, t, a.dead, AddI());
    o.remaining = tree(shi, t, a.remaining, AddI());
    o.no_episode = tree(shi, t, a.none, AddI());
    o.ret_sum = tree(shd, t, a.ret, AddD());
    o.ret2_sum = tree(shd, t, a.ret2, AddD());
    o.ret_min = tree(shd, t, a.mn, MinD());
    o.ret_max = tree(shd, t, a.mx, MaxD());
    if (t == 0) out[row] = o;
}

}  // namespace evxe

namespace {
using evxh::blocks;
using evxh::fail;
using evxh::failf;
using evxh::hip_status;
int check_ep(const evx_episodes* ep, const char* who) {
    if (!ep) return failf(-22, "%s: NULL episode descriptor", who);
    if (ep->E < 1) return failf(-22, "%s: E must be >= 1", who);
    if (!ep->ret || !ep->len || !ep->w_n || !ep->w_len || !ep->w_evac || !ep->w_dead || !ep->w_ret || !ep->w_ret2 ||
        !ep->w_min || !ep->w_max || !ep->last_ret || !ep->last_len || !ep->last_evac || !ep->last_dead ||
        !ep->n_total)
        return failf(-22, "%s: NULL episode buffer", who);
    if (ep->tab_slots < 0 || (ep->tab_slots > 0 && (!ep->tab_ret || !ep->tab_len || !ep->tab_evac || !ep->tab_dead)))
        return failf(-22, "%s: episode table slots without its buffers", who);
    return 0;
}
}  // namespace

extern "C" {

const char* evx_episode_last_error(void) { return evxh::g_err; }

int evx_episode_init(const evx_episodes* ep, void* stream) {
    if (int rc = check_ep(ep, "episode_init")) return rc;
    hipLaunchKernelGGL(evxe::episode_clear_kernel, dim3(blocks(ep->E, evxe::NT)), dim3(evxe::NT), 0,
                       (hipStream_t)stream, *ep, 1);
    return hip_status("episode_init");
}

int evx_episode_update(const evx_episodes* ep, const double* reward, const uint8_t* done, const int32_t* counts,
                       int64_t cap, void* stream) {
    if (int rc = check_ep(ep, "episode_update")) return rc;
    if (!reward || !done || !counts) return fail(-22, "episode_update: NULL reward, done or counts");
    hipLaunchKernelGGL(evxe::episode_update_kernel, dim3(blocks(ep->E, evxe::NT)), dim3(evxe::NT), 0,
                       (hipStream_t)stream, *ep, reward, done, counts, cap);
    return hip_status("episode_update");
}

int evx_episode_discard(const evx_episodes* ep, const uint8_t* mask, void* stream) {
    if (int rc = check_ep(ep, "episode_discard")) return rc;
    hipLaunchKernelGGL(evxe::episode_discard_kernel, dim3(blocks(ep->E, evxe::NT)), dim3(evxe::NT), 0,
                       (hipStream_t)stream, *ep, mask);
    return hip_status("episode_discard");
}

int evx_episode_reduce(const evx_episodes* ep, const int32_t* layout_idx, int32_t n_layouts, int64_t cap,
                       evx_episode_row* out, int32_t clear, void* stream) {
    if (int rc = check_ep(ep, "episode_reduce")) return rc;
    if (int rc = evxr::check_rows("episode_reduce", out, n_layouts, layout_idx)) return rc;
    return evxr::reduce_rows("episode_reduce", stream, clear, evxe::episode_reduce_kernel, evxe::episode_clear_kernel,
                             evxe::NT, *ep, layout_idx, n_layouts, cap, out);
}

}  // extern "C"
