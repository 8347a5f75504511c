// The span reduce of the per-env accumulators (episode.hip, health.hip, lstats.hip's value probe):
// what the three reduce kernels and their entry points have in common. Each family keeps its own
// row struct and its own gather loop over its fields; the order, the row filter, the tree and the
// entry points' refusals are here.
//
// One workgroup of RT threads per output row (row r < n_layouts: the envs of layout r; row
// n_layouts: all). Summation order (stated in evacx.h): thread t adds its row's envs t, t + RT,
// t + 2 RT, ... in ascending env order starting from 0; the RT thread sums are then added pairwise
// in LDS, s[t] = s[t] + s[t + h] for h = RT/2, RT/4, ..., 1. An env that is not of the row adds
// nothing (it is skipped, not added as zero: -0.0 stays out of it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "evacx.h"
#include "evx_host.h"

namespace evxr {

constexpr int RT = EVX_EPISODE_REDUCE_SPAN;  // the reduce's workgroup: envs per pass

// does env e add to this row?
__device__ __forceinline__ bool in_row(const int32_t* layout_idx, int n_layouts, int row, int e) {
    return !(row < n_layouts && (layout_idx ? layout_idx[e] : 0) != row);
}

struct AddI {
    __device__ int64_t operator()(int64_t a, int64_t b) const { return a + b; }
};
struct AddD {
    __device__ double operator()(double a, double b) const { return a + b; }
};
struct MinD {
    __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};
struct MaxD {
    __device__ double operator()(double a, double b) const { return b > a ? b : a; }
};
// s[t] = op(s[t], s[t + h]) for h = RT/2 .. 1; every thread returns s[0]
template <typename T, typename Op>
__device__ __forceinline__ T tree(T* s, int t, T v, Op op) {
    s[t] = v;
    __syncthreads();
    for (int h = RT / 2; h > 0; h >>= 1) {
        if (t < h) s[t] = op(s[t], s[t + h]);
        __syncthreads();
    }
    const T r = s[0];
    __syncthreads();
    return r;
}

// The refusals every reduce entry point shares (who: the entry's name in the error text).
inline int check_rows(const char* who, const void* out, int32_t n_layouts, const int32_t* layout_idx) {
    if (!out) return evxh::failf(-22, "%s: NULL output rows", who);
    if (n_layouts < 1 || n_layouts > 65535) return evxh::failf(-22, "%s: n_layouts must be 1..65535", who);
    if (n_layouts > 1 && !layout_idx) return evxh::failf(-22, "%s: several layouts need layout_idx", who);
    return 0;
}

// Launches the family's reduce kernel, reduce(d, layout_idx, n_layouts, more...), one workgroup per
// row, and with `clear` its clear kernel, clear_k(d, 0) over d.E envs in workgroups of clear_nt,
// after every row's workgroup has read the window (stream order).
template <class D, class RK, class CK, class... More>
inline int reduce_rows(const char* who, void* stream, int32_t clear, RK reduce, CK clear_k, int clear_nt, const D& d,
                       const int32_t* layout_idx, int32_t n_layouts, More... more) {
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reduce, dim3((unsigned)n_layouts + 1), dim3(RT), 0, st, d, layout_idx, (int)n_layouts, more...);
    if (int rc = evxh::hip_status(who)) return rc;
    if (!clear) return 0;
    hipLaunchKernelGGL(clear_k, dim3(evxh::blocks(d.E, clear_nt)), dim3(clear_nt), 0, st, d, 0);
    char what[64];
    snprintf(what, sizeof(what), "%s (clear)", who);
    return evxh::hip_status(what);
}

}  // namespace evxr
