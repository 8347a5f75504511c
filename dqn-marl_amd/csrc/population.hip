// Replay rings of a population of independent learners (evacx/population.py): `nets` uniform rings of
// one capacity, every array of evx_replay one allocation [nets][capacity] (ring k's arrays start
// k * capacity slots after ring 0's, which evx_replay points at), pushed and sampled in one launch each.
//   evx_replay_push_blocks   -> evx_replay_push_term of rows [k n, (k + 1) n) into ring k, every k
//   evx_replay_sample_blocks -> evx_replay_sample(ring k, size, B, seed, offset + k B) into rows
//                               [k B, (k + 1) B), every k
//   evx_replay_sample_nstep_blocks -> the same draws, each followed by evx_replay_nstep's chain on ring k
//                               with member k's own depth and discount, in the same launch
// Every member pushes the same number of rows per step, so one pos and one size serve all rings.
// The draws are evx_draws.h's keyed Feistel permutation, as the single ring's sampler takes them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "evacx.h"
#include "evx_host.h"
#include "evx_draws.h"

using evxh::fail;
using evxh::hip_status;

namespace evxp {

using namespace evxd;

// row g n + i -> ring g, slot (pos + i) mod capacity; the team reward / done of the row's env
__global__ __launch_bounds__(256) void push_blocks_kernel(evx_replay rp, const evx_obs* __restrict__ s,
                                                          const evx_obs* __restrict__ s2,
                                                          const evx_obs* __restrict__ s2_term,
                                                          const int32_t* __restrict__ a,
                                                          const double* __restrict__ r_env,
                                                          const uint8_t* __restrict__ done_env, int n,
                                                          int agents_per_env, int64_t pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t g = blockIdx.y;
    const int64_t row = g * n + i;
    const int64_t slot = g * rp.capacity + (pos + i) % rp.capacity;
    const int64_t e = row / agents_per_env;
    rp.s[slot] = s[row];
    rp.s2[slot] = (s2_term && done_env[e]) ? s2_term[row] : s2[row];
    rp.a[slot] = a[row];
    rp.r[slot] = (float)r_env[e];
    rp.done[slot] = done_env[e];
}

// draw i of ring g: replay_sample_kernel's (csrc/qnet.hip) over [0, size) under (seed, offset + g B)
__global__ __launch_bounds__(256) void sample_blocks_kernel(evx_replay rp, int64_t size, int B, uint64_t seed,
                                                            uint64_t offset, evx_obs* __restrict__ s,
                                                            evx_obs* __restrict__ s2, int32_t* __restrict__ a,
                                                            float* __restrict__ r, uint8_t* __restrict__ done) {
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= B) return;
    const int64_t g = blockIdx.y;
    const int64_t i = g * B + i0;
    const perm_key pk = make_perm_key((uint64_t)size, seed, offset + (uint64_t)g * (uint64_t)B, 0u);
    const int64_t j = g * rp.capacity + (int64_t)perm_apply(pk, (uint64_t)i0, (uint64_t)size);
    s[i] = rp.s[j];
    s2[i] = rp.s2[j];
    a[i] = rp.a[j];
    r[i] = rp.r[j];
    done[i] = rp.done[j];
}

// evx_replay_sample_nstep_blocks: a depth and a discount per ring, by value
struct NstepNets {
    int32_t n[64];
    float gamma[64];
};
// sample_blocks_kernel's draw j0 of ring g, then replay_nstep_kernel's chain (csrc/qnet.hip) from it on
// ring g with n[g] and gamma[g]: all f32, R + g * r a multiply and an add (-ffp-contract=off), int64
// slot arithmetic. j0 < size <= capacity, and every later slot is taken mod capacity.
__global__ __launch_bounds__(256) void sample_nstep_blocks_kernel(evx_replay rp, int64_t size, int B, uint64_t seed,
                                                                  uint64_t offset, int64_t base, int64_t count,
                                                                  int64_t stride, NstepNets nn,
                                                                  evx_obs* __restrict__ s, evx_obs* __restrict__ s2,
                                                                  int32_t* __restrict__ a, float* __restrict__ r,
                                                                  uint8_t* __restrict__ done,
                                                                  float* __restrict__ gamma_row,
                                                                  int32_t* __restrict__ len,
                                                                  int64_t* __restrict__ idx_out) {
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= B) return;
    const int64_t g = blockIdx.y;
    const int64_t i = g * B + i0;
    const perm_key pk = make_perm_key((uint64_t)size, seed, offset + (uint64_t)g * (uint64_t)B, 0u);
    const int64_t C = rp.capacity;
    const int64_t j0 = (int64_t)perm_apply(pk, (uint64_t)i0, (uint64_t)size);
    const int64_t ring = g * C;
    const int n_step = nn.n[g];
    const float gamma = nn.gamma[g];
    s[i] = rp.s[ring + j0];
    a[i] = rp.a[ring + j0];
    int64_t d0 = j0 - base;
    if (d0 < 0) d0 += C;
    int64_t j = j0;
    float R = rp.r[ring + j0], gm = gamma;
    uint8_t dn = rp.done[ring + j0];
    int L = 1;
    while (L < n_step && !dn && d0 + (int64_t)L * stride < count) {
        j = (j0 + (int64_t)L * stride) % C;
        R = R + gm * rp.r[ring + j];
        gm = gm * gamma;
        dn = rp.done[ring + j];
        L++;
    }
    r[i] = R;
    gamma_row[i] = gm;
    done[i] = dn;
    s2[i] = rp.s2[ring + j];
    if (len) len[i] = L;
    if (idx_out) idx_out[i] = j0;
}

static int nets_check(const char* bad, int32_t nets) { return nets < 1 || nets > 64 ? fail(-22, bad) : 0; }

}  // namespace evxp

extern "C" {

int evx_replay_push_blocks(const evx_replay* rp, const evx_obs* s, const evx_obs* s2, const evx_obs* s2_term,
                           const int32_t* a, const double* r_env, const uint8_t* done_env, int32_t n, int32_t nets,
                           int32_t agents_per_env, int64_t pos, void* stream) {
    if (!rp || !s || !s2 || !a || !r_env || !done_env) return fail(-22, "replay_push_blocks: NULL argument");
    if (!rp->s || !rp->s2 || !rp->a || !rp->r || !rp->done) return fail(-22, "replay_push_blocks: NULL ring array");
    if (int rc = evxp::nets_check("replay_push_blocks: nets must be 1..64", nets)) return rc;
    if (n < 0 || (n & 1)) return fail(-22, "replay_push_blocks: rows per ring must be even and >= 0");
    if (rp->capacity < 1 || rp->capacity < n) return fail(-22, "replay_push_blocks: the capacity does not hold n rows");
    if (agents_per_env < 1 || n % agents_per_env)
        return fail(-22, "replay_push_blocks: rows per ring must be a multiple of agents_per_env");
    if (pos < 0 || pos >= rp->capacity) return fail(-22, "replay_push_blocks: pos outside [0, capacity)");
    if (n == 0) return 0;
    hipLaunchKernelGGL(evxp::push_blocks_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nets), dim3(256), 0,
                       (hipStream_t)stream, *rp, s, s2, s2_term, a, r_env, done_env, n, agents_per_env, pos);
    return hip_status("replay_push_blocks");
}

int evx_replay_sample_blocks(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                             uint64_t offset, evx_obs* s, evx_obs* s2, int32_t* a, float* r, uint8_t* done,
                             void* stream) {
    if (!rp || !s || !s2 || !a || !r || !done) return fail(-22, "replay_sample_blocks: NULL argument");
    if (!rp->s || !rp->s2 || !rp->a || !rp->r || !rp->done) return fail(-22, "replay_sample_blocks: NULL ring array");
    if (int rc = evxp::nets_check("replay_sample_blocks: nets must be 1..64", nets)) return rc;
    if (B < 0 || (B & 1)) return fail(-22, "replay_sample_blocks: B must be even and >= 0");
    if (size < 1 || size > rp->capacity) return fail(-22, "replay_sample_blocks: size outside [1, capacity]");
    if (B > size) return fail(-22, "replay_sample_blocks: sample larger than a ring's population (random.sample)");
    if (B == 0) return 0;
    hipLaunchKernelGGL(evxp::sample_blocks_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)nets), dim3(256), 0,
                       (hipStream_t)stream, *rp, size, B, seed, offset, s, s2, a, r, done);
    return hip_status("replay_sample_blocks");
}

int evx_replay_sample_nstep_blocks(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                                   uint64_t offset, int64_t base, int64_t count, int64_t stride,
                                   const int32_t* n_step, const float* gamma, evx_obs* s, evx_obs* s2, int32_t* a,
                                   float* r, uint8_t* done, float* gamma_row, int32_t* len, int64_t* idx_out,
                                   void* stream) {
    if (!rp || !n_step || !gamma || !s || !s2 || !a || !r || !done || !gamma_row)
        return fail(-22, "replay_sample_nstep_blocks: NULL argument");
    if (!rp->s || !rp->s2 || !rp->a || !rp->r || !rp->done)
        return fail(-22, "replay_sample_nstep_blocks: NULL ring array");
    if (int rc = evxp::nets_check("replay_sample_nstep_blocks: nets must be 1..64", nets)) return rc;
    if (B < 0 || (B & 1)) return fail(-22, "replay_sample_nstep_blocks: B must be even and >= 0");
    if (size < 1 || size > rp->capacity) return fail(-22, "replay_sample_nstep_blocks: size outside [1, capacity]");
    if (B > size)
        return fail(-22, "replay_sample_nstep_blocks: sample larger than a ring's population (random.sample)");
    if (count < 0 || count > rp->capacity) return fail(-22, "replay_sample_nstep_blocks: count outside [0, capacity]");
    if (base < 0 || base >= rp->capacity) return fail(-22, "replay_sample_nstep_blocks: base outside [0, capacity)");
    if (stride < 1) return fail(-22, "replay_sample_nstep_blocks: stride must be >= 1");
    evxp::NstepNets nn{};
    for (int k = 0; k < nets; k++) {
        if (n_step[k] < 1 || n_step[k] > EVX_NSTEP_MAX)
            return fail(-22, "replay_sample_nstep_blocks: n_step must be 1..EVX_NSTEP_MAX (32)");
        if (!std::isfinite(gamma[k])) return fail(-22, "replay_sample_nstep_blocks: gamma must be finite");
        nn.n[k] = n_step[k];
        nn.gamma[k] = gamma[k];
    }
    if (B == 0) return 0;
    // a stride beyond the ring never finds a successor inside the range (count <= capacity): the
    // capacity stands for it, so L * stride cannot overflow
    hipLaunchKernelGGL(evxp::sample_nstep_blocks_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)nets), dim3(256),
                       0, (hipStream_t)stream, *rp, size, B, seed, offset, base, count,
                       std::min<int64_t>(stride, rp->capacity), nn, s, s2, a, r, done, gamma_row, len, idx_out);
    return hip_status("replay_sample_nstep_blocks");
}

}  // extern "C"
