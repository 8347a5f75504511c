// MI355X (gfx950) learner diagnostics: statistics of the learn step's sampled batch and a value
// probe, kept on the device.
//
// The learn chain leaves Q, the target's Q, the batch, the loss and the gradient norm in the
// learner's own buffers until its next step; the act leaves the Q row every action was chosen from.
// Nothing of it reaches the host inside a step, so the quantities Double-Q, the Huber loss and the
// soft target are there to control are folded here, per net and per env, and read at the log
// interval. Both families only read their inputs: the learner's and the env's numbers are the same
// bits with them on or off.
//
// Learn statistics: two launches per update. The rows kernel (one thread per row, 256-row blocks,
// blockIdx.y = net) takes each row through the TD kernels' expressions, adds the integer counts with
// integer atomics (exact in any order) and leaves each block's f64 sums -- one fixed LDS tree -- in
// the caller's workspace; one workgroup per net then adds the blocks in ascending order and takes
// the step's loss and norm. No float atomics.
// Value probe: one thread per env, an env's numbers depend on its own step sequence only; the only
// sums over envs are the reduce's, in evx_episode_reduce's order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "evacx.h"
#include "evx_host.h"
#include "evx_reduce.h"

namespace evxl {

constexpr int NT = 256;                      // rows per block; envs per block of the probe's kernels
constexpr int MAXA = EVX_LSTATS_MAX_A;
constexpr int NBK = EVX_LSTATS_TD_BUCKETS;
constexpr int WF = EVX_LSTATS_WS_FIELDS;
using evxr::RT, evxr::in_row, evxr::tree, evxr::AddI, evxr::AddD, evxr::MinD, evxr::MaxD;
// the block's integer counters in LDS: rows_bad, n_done, n_greedy, act_hist[MAXA], td_hist[NBK]
constexpr int C_BAD = 0, C_DONE = 1, C_GREEDY = 2, C_ACT = 3, C_TD = C_ACT + MAXA, NCNT = C_TD + NBK;

struct RowIn {
    const float* Q;
    const float* Qt;
    const int32_t* act;
    const float* rew;
    const uint8_t* done;
    const int32_t* sel;
    const float* gamma_row;
    float* d_out;
    float gamma;
    int B;
};

__device__ __forceinline__ void add_i64(int64_t* p, int64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__global__ __launch_bounds__(NT) void lstats_rows_kernel(evx_lstats ls, RowIn in, double* __restrict__ ws) {
    __shared__ double red[WF][NT];  // the ten fields' trees side by side: one pass of barriers
    __shared__ int32_t cnt[NCNT];
    const int t = threadIdx.x, g = blockIdx.y, A = ls.A, B = in.B;
    for (int k = t; k < NCNT; k += NT) cnt[k] = 0;
    __syncthreads();
    const int i = blockIdx.x * NT + t;
    double vq = 0.0, vqmax = 0.0, vy = 0.0, vd = 0.0, vabs = 0.0, vd2 = 0.0, vrew = 0.0;
    double mabs = -INFINITY, mq = -INFINITY, nq = INFINITY;
    if (i < B) {
        const size_t row = (size_t)g * B + i;
        const float* q_row = in.Q + row * A;
        const float* t_row = in.Qt + row * A;
        const int ai = in.act[row];
        const int a = min(max(ai, 0), A - 1);
        const float q = q_row[a];
        float qmax = q_row[0], qmin = q_row[0];
        int jmax = 0;
        for (int j = 1; j < A; j++) {
            const float v = q_row[j];
            if (v > qmax) {
                qmax = v;
                jmax = j;
            }
            if (v < qmin) qmin = v;
        }
        float tv;
        if (in.sel) {
            tv = t_row[min(max(in.sel[row], 0), A - 1)];
        } else {
            tv = t_row[0];
            for (int j = 1; j < A; j++)
                if (t_row[j] > tv) tv = t_row[j];
        }
        const float rw = in.rew[row];
        const uint8_t dn = in.done[row];
        const float gm = in.gamma_row ? in.gamma_row[row] : in.gamma;
        const float y = rw + (gm * tv) * (dn ? 0.f : 1.f);
        const float d = q - y;
        const bool bad = !(isfinite(q) && isfinite(qmax) && isfinite(y));
        if (in.d_out) in.d_out[row] = bad ? __uint_as_float(0x7fc00000u) : d;
        if (bad) {
            atomicAdd(&cnt[C_BAD], 1);
        } else {
            const float ad = fabsf(d);
            vq = (double)q;
            vqmax = (double)qmax;
            vy = (double)y;
            vd = (double)d;
            vabs = (double)ad;
            vd2 = vd * vd;
            vrew = (double)rw;
            mabs = vabs;
            mq = vqmax;
            nq = (double)qmin;
            if (dn) atomicAdd(&cnt[C_DONE], 1);
            if (ai == jmax) atomicAdd(&cnt[C_GREEDY], 1);
            atomicAdd(&cnt[C_ACT + a], 1);
            const int k = min(max((int)(__float_as_uint(ad) >> 23) - 103, 0), NBK - 1);
            atomicAdd(&cnt[C_TD + k], 1);
        }
    }
    red[0][t] = vq;
    red[1][t] = vqmax;
    red[2][t] = vy;
    red[3][t] = vd;
    red[4][t] = vabs;
    red[5][t] = vd2;
    red[6][t] = vrew;
    red[7][t] = mabs;
    red[8][t] = mq;
    red[9][t] = nq;
    __syncthreads();
    // s[t] = s[t] + s[t + h] for h = 128 .. 1 (fields 7, 8: the larger; field 9: the smaller)
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int f = 0; f < 7; f++) red[f][t] = red[f][t] + red[f][t + h];
            red[7][t] = red[7][t + h] > red[7][t] ? red[7][t + h] : red[7][t];
            red[8][t] = red[8][t + h] > red[8][t] ? red[8][t + h] : red[8][t];
            red[9][t] = red[9][t + h] < red[9][t] ? red[9][t + h] : red[9][t];
        }
        __syncthreads();
    }
    if (t < WF) ws[((size_t)g * gridDim.x + blockIdx.x) * WF + t] = red[t][0];
    // the block's counts (cnt is complete: the tree's barriers followed every LDS atomic)
    if (t < NCNT) {
        const int32_t c = cnt[t];
        if (c) {
            int64_t* dst;
            if (t == C_BAD)
                dst = ls.rows_bad + g;
            else if (t == C_DONE)
                dst = ls.n_done + g;
            else if (t == C_GREEDY)
                dst = ls.n_greedy + g;
            else if (t < C_TD)
                dst = ls.act_hist + (size_t)g * MAXA + (t - C_ACT);
            else
                dst = ls.td_hist + (size_t)g * NBK + (t - C_TD);
            add_i64(dst, c);
        }
    }
}

// One workgroup per net. The net's block partials are staged in LDS FCH blocks at a time (coalesced
// loads; a serial walk over global memory pays its latency once per block), then thread f < 7 adds
// field f's block sums in ascending block order onto 0.0 and the total to the window; threads 7..9
// take the extremes; thread 10 the step.
constexpr int FCH = 512;  // blocks per staged chunk: 40 KB of LDS
__global__ __launch_bounds__(NT) void lstats_finish_kernel(evx_lstats ls, const double* __restrict__ ws, int nb, int B,
                                                           const float* __restrict__ loss,
                                                           const float* __restrict__ norm, float max_norm) {
    __shared__ double st[FCH * WF];
    const int g = blockIdx.x, t = threadIdx.x;
    const double* p = ws + (size_t)g * nb * WF;
    double acc = t < 7 ? 0.0 : t == 9 ? (double)INFINITY : (double)-INFINITY;
    for (int b0 = 0; b0 < nb; b0 += FCH) {
        const int n = min(FCH, nb - b0);
        for (int k = t; k < n * WF; k += NT) st[k] = p[(size_t)b0 * WF + k];
        __syncthreads();
        if (t < 7) {
            for (int b = 0; b < n; b++) acc = acc + st[b * WF + t];
        } else if (t < 9) {
            for (int b = 0; b < n; b++) acc = st[b * WF + t] > acc ? st[b * WF + t] : acc;
        } else if (t == 9) {
            for (int b = 0; b < n; b++) acc = st[b * WF + 9] < acc ? st[b * WF + 9] : acc;
        }
        __syncthreads();
    }
    if (t < 7) {
        double* dst = t == 0 ? ls.s_q : t == 1 ? ls.s_qmax : t == 2 ? ls.s_y : t == 3 ? ls.s_d
                    : t == 4 ? ls.s_absd : t == 5 ? ls.s_d2 : ls.s_rew;
        dst[g] = dst[g] + acc;
    } else if (t < 9) {
        double* dst = t == 7 ? ls.max_absd : ls.max_q;
        if (acc > dst[g]) dst[g] = acc;
    } else if (t == 9) {
        if (acc < ls.min_q[g]) ls.min_q[g] = acc;
    } else if (t == 10) {
        ls.rows[g] += B;
        ls.steps[g] += 1;
        const float l = loss ? loss[g] : 0.f, n = norm ? norm[g] : 0.f;
        if (isfinite(l) && isfinite(n)) {
            if (loss) {
                ls.s_loss[g] = ls.s_loss[g] + (double)l;
                if ((double)l > ls.max_loss[g]) ls.max_loss[g] = (double)l;
            }
            if (norm) {
                ls.s_norm[g] = ls.s_norm[g] + (double)n;
                if ((double)n > ls.max_norm[g]) ls.max_norm[g] = (double)n;
                if (max_norm > 0.f && n > max_norm) ls.n_clipped[g] += 1;
            }
        } else {
            ls.steps_bad[g] += 1;
        }
    }
}

__global__ __launch_bounds__(NT) void lstats_clear_kernel(evx_lstats ls) {
    const int k = blockIdx.x * NT + threadIdx.x;
    const int n = ls.nets;
    if (k < n) {
        ls.steps[k] = 0;
        ls.steps_bad[k] = 0;
        ls.rows[k] = 0;
        ls.rows_bad[k] = 0;
        ls.n_done[k] = 0;
        ls.n_greedy[k] = 0;
        ls.n_clipped[k] = 0;
        ls.s_q[k] = 0.0;
        ls.s_qmax[k] = 0.0;
        ls.s_y[k] = 0.0;
        ls.s_d[k] = 0.0;
        ls.s_absd[k] = 0.0;
        ls.s_d2[k] = 0.0;
        ls.s_rew[k] = 0.0;
        ls.s_loss[k] = 0.0;
        ls.s_norm[k] = 0.0;
        ls.max_absd[k] = -INFINITY;
        ls.max_q[k] = -INFINITY;
        ls.min_q[k] = INFINITY;
        ls.max_loss[k] = -INFINITY;
        ls.max_norm[k] = -INFINITY;
    }
    if (k < n * MAXA) ls.act_hist[k] = 0;
    if (k < n * NBK) ls.td_hist[k] = 0;
}

// ------------------------------------------------------------------ value probe
__global__ __launch_bounds__(NT) void vprobe_update_kernel(evx_vprobe vp, const float* __restrict__ Q,
                                                            const int32_t* __restrict__ act,
                                                            const double* __restrict__ reward,
                                                            const uint8_t* __restrict__ done, double gamma) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= vp.E) return;
    double q0, g, disc;
    int32_t len;
    if (!vp.open[e]) {
        double s = 0.0;
        for (int r = 0; r < vp.R; r++) {
            const size_t row = (size_t)e * vp.R + r;
            s = s + (double)Q[row * vp.A + min(max(act[row], 0), vp.A - 1)];
        }
        q0 = s / (double)vp.R;
        g = 0.0;
        disc = 1.0;
        len = 0;
        vp.q0[e] = q0;
    } else {
        q0 = vp.q0[e];
        g = vp.g[e];
        disc = vp.disc[e];
        len = vp.len[e];
    }
    g = g + disc * reward[e];
    disc = disc * gamma;
    len += 1;
    vp.g[e] = g;
    vp.disc[e] = disc;
    vp.len[e] = len;
    if (!done[e]) {
        vp.open[e] = 1;
        return;
    }
    if (!isfinite(q0)) {
        vp.w_bad[e] += 1;
    } else {
        const double err = q0 - g;
        vp.w_n[e] += 1;
        vp.w_q[e] = vp.w_q[e] + q0;
        vp.w_g[e] = vp.w_g[e] + g;
        vp.w_e[e] = vp.w_e[e] + err;
        vp.w_e2[e] = vp.w_e2[e] + err * err;
        vp.w_q2[e] = vp.w_q2[e] + q0 * q0;
        vp.w_g2[e] = vp.w_g2[e] + g * g;
        vp.w_qg[e] = vp.w_qg[e] + q0 * g;
        if (err < vp.w_emin[e]) vp.w_emin[e] = err;
        if (err > vp.w_emax[e]) vp.w_emax[e] = err;
    }
    vp.open[e] = 0;
}

__global__ __launch_bounds__(NT) void vprobe_discard_kernel(evx_vprobe vp, const uint8_t* __restrict__ mask) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= vp.E || (mask && !mask[e])) return;
    vp.open[e] = 0;
}

__global__ __launch_bounds__(NT) void vprobe_clear_kernel(evx_vprobe vp, int all) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= vp.E) return;
    vp.w_n[e] = 0;
    vp.w_bad[e] = 0;
    vp.w_q[e] = 0.0;
    vp.w_g[e] = 0.0;
    vp.w_e[e] = 0.0;
    vp.w_e2[e] = 0.0;
    vp.w_q2[e] = 0.0;
    vp.w_g2[e] = 0.0;
    vp.w_qg[e] = 0.0;
    vp.w_emin[e] = INFINITY;
    vp.w_emax[e] = -INFINITY;
    if (all) {
        vp.open[e] = 0;
        vp.q0[e] = 0.0;
        vp.g[e] = 0.0;
        vp.disc[e] = 1.0;
        vp.len[e] = 0;
    }
}

// One workgroup per output row, in the order of evx_reduce.h.
__global__ __launch_bounds__(RT) void vprobe_reduce_kernel(evx_vprobe vp, const int32_t* __restrict__ layout_idx,
                                                           int n_layouts, evx_vprobe_row* __restrict__ out) {
    __shared__ double shd[RT];
    __shared__ int64_t shi[RT];
    const int row = blockIdx.x, t = threadIdx.x;
    int64_t n = 0, bad = 0, open = 0;
    double q = 0.0, g = 0.0, e1 = 0.0, e2 = 0.0, q2 = 0.0, g2 = 0.0, qg = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int e = t; e < vp.E; e += RT) {
        if (!in_row(layout_idx, n_layouts, row, e)) continue;
        n += vp.w_n[e];
        bad += vp.w_bad[e];
        open += vp.open[e] ? 1 : 0;
        q = q + vp.w_q[e];
        g = g + vp.w_g[e];
        e1 = e1 + vp.w_e[e];
        e2 = e2 + vp.w_e2[e];
        q2 = q2 + vp.w_q2[e];
        g2 = g2 + vp.w_g2[e];
        qg = qg + vp.w_qg[e];
        const double lo = vp.w_emin[e], hi = vp.w_emax[e];
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
    }
    evx_vprobe_row o;
    o.probes = tree(shi, t, n, AddI());
    o.bad = tree(shi, t, bad, AddI());
    o.open = tree(shi, t, open, AddI());
    o.q_sum = tree(shd, t, q, AddD());
    o.g_sum = tree(shd, t, g, AddD());
    o.e_sum = tree(shd, t, e1, AddD());
    o.e2_sum = tree(shd, t, e2, AddD());
    o.q2_sum = tree(shd, t, q2, AddD());
    o.g2_sum = tree(shd, t, g2, AddD());
    o.qg_sum = tree(shd, t, qg, AddD());
    o.e_min = tree(shd, t, mn, MinD());
    o.e_max = tree(shd, t, mx, MaxD());
    if (t == 0) out[row] = o;
}

}  // namespace evxl

namespace {
using evxh::blocks;
using evxh::fail;
using evxh::failf;
using evxh::hip_status;

int check_ls(const evx_lstats* ls, const char* who) {
    if (!ls) return failf(-22, "%s: NULL statistics descriptor", who);
    if (ls->nets < 1 || ls->nets > 64) return failf(-22, "%s: nets must be 1..64", who);
    if (ls->A < 1 || ls->A > EVX_LSTATS_MAX_A) return failf(-22, "%s: A must be 1..%d", who, EVX_LSTATS_MAX_A);
    if (!ls->steps || !ls->steps_bad || !ls->rows || !ls->rows_bad || !ls->n_done || !ls->n_greedy ||
        !ls->n_clipped || !ls->act_hist || !ls->td_hist || !ls->s_q || !ls->s_qmax || !ls->s_y || !ls->s_d ||
        !ls->s_absd || !ls->s_d2 || !ls->s_rew || !ls->s_loss || !ls->s_norm || !ls->max_absd || !ls->max_q ||
        !ls->min_q || !ls->max_loss || !ls->max_norm)
        return failf(-22, "%s: NULL statistics buffer", who);
    return 0;
}

int check_vp(const evx_vprobe* vp, const char* who) {
    if (!vp) return failf(-22, "%s: NULL probe descriptor", who);
    if (vp->E < 1 || vp->R < 1 || vp->A < 1) return failf(-22, "%s: E, R and A must be >= 1", who);
    if (vp->A > EVX_LSTATS_MAX_A) return failf(-22, "%s: A must be <= %d", who, EVX_LSTATS_MAX_A);
    if ((int64_t)vp->E * vp->R > INT32_MAX) return failf(-22, "%s: E * R beyond 2^31 - 1", who);
    if (!vp->open || !vp->q0 || !vp->g || !vp->disc || !vp->len || !vp->w_n || !vp->w_bad || !vp->w_q || !vp->w_g ||
        !vp->w_e || !vp->w_e2 || !vp->w_q2 || !vp->w_g2 || !vp->w_qg || !vp->w_emin || !vp->w_emax)
        return failf(-22, "%s: NULL probe buffer", who);
    return 0;
}
}  // namespace

extern "C" {

const char* evx_lstats_last_error(void) { return evxh::g_err; }

int64_t evx_lstats_ws_doubles(int32_t B, int32_t nets) {
    if (B < 1 || nets < 1) return 0;
    return (int64_t)nets * ((B + evxl::NT - 1) / evxl::NT) * EVX_LSTATS_WS_FIELDS;
}

int evx_lstats_init(const evx_lstats* ls, void* stream) {
    if (int rc = check_ls(ls, "lstats_init")) return rc;
    hipLaunchKernelGGL(evxl::lstats_clear_kernel, dim3(blocks((int64_t)ls->nets * EVX_LSTATS_TD_BUCKETS, evxl::NT)),
                       dim3(evxl::NT), 0, (hipStream_t)stream, *ls);
    return hip_status("lstats_init");
}

int evx_lstats_update(const evx_lstats* ls, const float* Q, const float* Qt, const int32_t* act, const float* rew,
                      const uint8_t* done, float gamma, int32_t B, const evx_td_opts* opt, const float* loss,
                      const float* norm, float max_norm, float* d_out, double* ws, int64_t ws_doubles, void* stream) {
    if (int rc = check_ls(ls, "lstats_update")) return rc;
    if (!Q || !Qt || !act || !rew || !done) return fail(-22, "lstats_update: NULL Q, Qt, act, rew or done");
    if (B < 1) return fail(-22, "lstats_update: B must be >= 1");
    if ((int64_t)B * ls->nets > INT32_MAX) return fail(-22, "lstats_update: nets * B beyond 2^31 - 1");
    if (!isfinite(gamma)) return fail(-22, "lstats_update: gamma is not finite");
    if (!ws) return fail(-22, "lstats_update: NULL workspace");
    if (ws_doubles < evx_lstats_ws_doubles(B, ls->nets))
        return fail(-22, "lstats_update: workspace smaller than evx_lstats_ws_doubles(B, nets)");
    evxl::RowIn in;
    in.Q = Q;
    in.Qt = Qt;
    in.act = act;
    in.rew = rew;
    in.done = done;
    in.sel = opt ? opt->sel : nullptr;
    in.gamma_row = opt ? opt->gamma_row : nullptr;
    in.d_out = d_out;
    in.gamma = gamma;
    in.B = B;
    const int nb = (B + evxl::NT - 1) / evxl::NT;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(evxl::lstats_rows_kernel, dim3((unsigned)nb, (unsigned)ls->nets), dim3(evxl::NT), 0, st, *ls, in,
                       ws);
    if (int rc = hip_status("lstats_update (rows)")) return rc;
    hipLaunchKernelGGL(evxl::lstats_finish_kernel, dim3((unsigned)ls->nets), dim3(evxl::NT), 0, st, *ls, ws, nb, B,
                       loss, norm, max_norm);
    return hip_status("lstats_update (finish)");
}

int evx_vprobe_init(const evx_vprobe* vp, void* stream) {
    if (int rc = check_vp(vp, "vprobe_init")) return rc;
    hipLaunchKernelGGL(evxl::vprobe_clear_kernel, dim3(blocks(vp->E, evxl::NT)), dim3(evxl::NT), 0,
                       (hipStream_t)stream, *vp, 1);
    return hip_status("vprobe_init");
}

int evx_vprobe_update(const evx_vprobe* vp, const float* Q, const int32_t* act, const double* reward,
                      const uint8_t* done, double gamma, void* stream) {
    if (int rc = check_vp(vp, "vprobe_update")) return rc;
    if (!Q || !act || !reward || !done) return fail(-22, "vprobe_update: NULL Q, act, reward or done");
    if (!isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return fail(-22, "vprobe_update: gamma must be in [0, 1]");
    hipLaunchKernelGGL(evxl::vprobe_update_kernel, dim3(blocks(vp->E, evxl::NT)), dim3(evxl::NT), 0,
                       (hipStream_t)stream, *vp, Q, act, reward, done, gamma);
    return hip_status("vprobe_update");
}

int evx_vprobe_discard(const evx_vprobe* vp, const uint8_t* mask, void* stream) {
    if (int rc = check_vp(vp, "vprobe_discard")) return rc;
    hipLaunchKernelGGL(evxl::vprobe_discard_kernel, dim3(blocks(vp->E, evxl::NT)), dim3(evxl::NT), 0,
                       (hipStream_t)stream, *vp, mask);
    return hip_status("vprobe_discard");
}

int evx_vprobe_reduce(const evx_vprobe* vp, const int32_t* layout_idx, int32_t n_layouts, evx_vprobe_row* out,
                      int32_t clear, void* stream) {
    if (int rc = check_vp(vp, "vprobe_reduce")) return rc;
    if (int rc = evxr::check_rows("vprobe_reduce", out, n_layouts, layout_idx)) return rc;
    return evxr::reduce_rows("vprobe_reduce", stream, clear, evxl::vprobe_reduce_kernel, evxl::vprobe_clear_kernel,
                             evxl::NT, *vp, layout_idx, n_layouts, out);
}

}  // extern "C"
