// Every entry of the uniform replay ring (DQNAgent.memory, agents/dqn_agent.py:88-99; compact
// observations, per-agent transitions that share their env's team reward / done): one ring's, and the
// _blocks entries of a population's `nets` rings of one capacity (evacx/population.py), every array of
// evx_replay one allocation [nets][capacity] (ring k's arrays start k * capacity slots after ring 0's,
// which evx_replay points at), pushed and sampled in one launch each; every member pushes the same
// number of rows per step, so one pos and one size serve all rings. The push rule, the row gather,
// the draws and the n-step chain are evx_ring.h's: a kernel here is index computation plus calls into it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "evacx.h"
#include "evx_host.h"
#include "evx_ring.h"

namespace evxq {

using namespace evxr;

// row g n + i -> ring g, slot (pos + i) mod capacity; the team reward / done of the row's env
// (n is a multiple of agents_per_env, so the env is g (n / agents_per_env) + i / agents_per_env).
// One ring: g = 0.
__global__ __launch_bounds__(256) void replay_push_kernel(evx_replay rp, const evx_obs* __restrict__ s,
                                                          const evx_obs* __restrict__ s2,
                                                          const evx_obs* __restrict__ s2_term, const int32_t* __restrict__ a,
                                                          const double* __restrict__ r_env,
                                                          const uint8_t* __restrict__ done_env, int n, int agents_per_env,
                                                          int64_t pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t g = blockIdx.y;
    ring_put(rp, g * rp.capacity + (pos + i) % rp.capacity, {s, s2, s2_term, a, r_env, done_env}, g * n + i,
             g * (n / agents_per_env) + i / agents_per_env);
}

// draw i0 of grid row g (evx_ring.h's mappings) into batch row g B + i0; idx_out: the ring-local slot
template <int MAP>
__global__ __launch_bounds__(256) void replay_sample_kernel(evx_replay rp, draw_args d, evx_obs* __restrict__ s,
                                                            evx_obs* __restrict__ s2, int32_t* __restrict__ a,
                                                            float* __restrict__ r, uint8_t* __restrict__ done,
                                                            int64_t* __restrict__ idx_out) {
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= d.B) return;
    const int g = (int)blockIdx.y;
    const int64_t i = (int64_t)g * d.B + i0;
    const int64_t j = draw_slot<MAP>(d, rp.capacity, i0, g);
    ring_take(rp, draw_ring<MAP>(rp.capacity, g) + j, rows{s, s2, a, r, done}, i);
    if (idx_out) idx_out[i] = j;
}

// One row per thread: the chain from the given slot. A slot index outside the ring is clamped into
// it (never read out of bounds).
__global__ __launch_bounds__(256) void replay_nstep_kernel(evx_replay rp, const int64_t* __restrict__ idx, int B,
                                                           int64_t base, int64_t count, int64_t stride, int n_step,
                                                           float gamma, evx_obs* __restrict__ s2,
                                                           float* __restrict__ r, uint8_t* __restrict__ done,
                                                           float* __restrict__ gamma_row, int32_t* __restrict__ len) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t j0 = min(max(idx[i], (int64_t)0), rp.capacity - 1);
    ring_chain(rp, 0, j0, base, count, stride, n_step, gamma, i, r, gamma_row, done, s2, len);
}

// The chains' depth and discount by value: one pair for every grid row (N = 1), or one per ring.
template <int N>
struct Nstep {
    int32_t n[N];
    float gamma[N];
};
// replay_sample_kernel's draw j0, s and a from it, then replay_nstep_kernel's chain from j0 on the
// draw's ring in the same launch. AGENTS: the stride is a multiple of nets for whole-env pushes, so
// every slot of a chain is the same agent's; in joint mode the agents of a draw share the env-steps,
// the push gave them the env's team reward and done flag, and so their chains have one length.
template <int MAP, int N>
__global__ __launch_bounds__(256) void replay_sample_nstep_kernel(
    evx_replay rp, draw_args d, int64_t base, int64_t count, int64_t stride, Nstep<N> ns,
    evx_obs* __restrict__ s, evx_obs* __restrict__ s2, int32_t* __restrict__ a, float* __restrict__ r,
    uint8_t* __restrict__ done, float* __restrict__ gamma_row, int32_t* __restrict__ len,
    int64_t* __restrict__ idx_out) {
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= d.B) return;
    const int g = (int)blockIdx.y;
    const int64_t i = (int64_t)g * d.B + i0;
    const int64_t j0 = draw_slot<MAP>(d, rp.capacity, i0, g), ring = draw_ring<MAP>(rp.capacity, g);
    s[i] = rp.s[ring + j0];
    a[i] = rp.a[ring + j0];
    const int k = N > 1 ? g : 0;
    ring_chain(rp, ring, j0, base, count, stride, ns.n[k], ns.gamma[k], i, r, gamma_row, done, s2, len);
    if (idx_out) idx_out[i] = j0;
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const evx_obs* __restrict__ src,
                                                          const int64_t* __restrict__ idx, int n,
                                                          evx_obs* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

}  // namespace evxq

namespace {

using evxh::fail;
using evxh::failf;
using evxh::hip_status;
using namespace evxr;

unsigned nblk(int64_t n) { return evxh::blocks(n, 256); }

// What a push of n rows at pos must satisfy before anything is launched (as evx_replay_push_blocks):
// n > capacity would let two threads write one slot, a pos outside the ring a slot outside it, and
// agents_per_env < 1 divides by zero on the device. 0: launch; 1: nothing to push; -22: refused.
int push_check(const char* who, const evx_replay* rp, const evx_obs* s, const evx_obs* s2, const int32_t* a,
               const double* r_env, const uint8_t* done_env, int32_t n, int32_t agents_per_env, int64_t pos) {
    if (!rp || rp->capacity <= 0) return failf(-22, "%s: bad ring (NULL, or capacity < 1)", who);
    if (int rc = ring_arrays_ok(who, rp)) return rc;
    if (n < 0) return failf(-22, "%s: n must be >= 0", who);
    if (n > rp->capacity) return failf(-22, "%s: the capacity does not hold n rows", who);
    if (pos < 0 || pos >= rp->capacity) return failf(-22, "%s: pos outside [0, capacity)", who);
    if (agents_per_env < 1 || n % agents_per_env) return failf(-22, "%s: n must be a multiple of agents_per_env >= 1", who);
    if (n == 0) return 1;
    if (!s || !s2 || !a || !r_env || !done_env) return failf(-22, "%s: NULL argument", who);
    return 0;
}

// n rows of each of `rings` rings at pos
int push_launch(const char* who, const evx_replay* rp, const push_src& src, int32_t n, int32_t rings,
                int32_t agents_per_env, int64_t pos, void* stream) {
    hipLaunchKernelGGL(evxq::replay_push_kernel, dim3(nblk(n), (unsigned)rings), dim3(256), 0, (hipStream_t)stream, *rp,
                       src.s, src.s2, src.s2_term, src.a, src.r_env, src.done_env, n, agents_per_env, pos);
    return hip_status(who);
}

// What the block rings' samplers share, after their own NULL-argument line.
int blocks_check(const char* who, const evx_replay* rp, int64_t size, int32_t B, int32_t nets) {
    if (int rc = ring_arrays_ok(who, rp)) return rc;
    if (nets < 1 || nets > 64) return failf(-22, "%s: nets must be 1..64", who);
    if (B < 0 || (B & 1)) return failf(-22, "%s: B must be even and >= 0", who);
    if (size < 1 || size > rp->capacity) return failf(-22, "%s: size outside [1, capacity]", who);
    if (B > size) return failf(-22, "%s: sample larger than a ring's population (random.sample)", who);
    return 0;
}

template <int MAP>
int sample_launch(const char* who, const evx_replay* rp, const draw_args& d, evx_obs* s, evx_obs* s2, int32_t* a,
                  float* r, uint8_t* done, int64_t* idx_out, void* stream) {
    hipLaunchKernelGGL(evxq::replay_sample_kernel<MAP>, dim3(nblk(d.B), (unsigned)d.nets), dim3(256), 0,
                       (hipStream_t)stream, *rp, d, s, s2, a, r, done, idx_out);
    return hip_status(who);
}

// evx_replay_sample_agents, and with joint evx_replay_sample_joint
int sample_agents(const char* who, int joint, const evx_replay* rp, int64_t size, int32_t B, int32_t nets,
                  uint64_t seed, uint64_t offset, evx_obs* s, evx_obs* s2, int32_t* a, float* r, uint8_t* done,
                  void* stream) {
    if (!rp || !s || !s2 || !a || !r || !done) return failf(-22, "%s: NULL argument", who);
    if (B <= 0) return 0;
    if (int rc = agents_ok(who, rp, size, B, nets, joint != 0)) return rc;
    return sample_launch<AGENTS>(who, rp, {0, size, B, nets, joint, seed, offset}, s, s2, a, r, done, nullptr, stream);
}

}  // namespace

extern "C" {

int evx_replay_push(const evx_replay* rp, const evx_obs* s, const evx_obs* s2, const int32_t* a, const double* r_env,
                    const uint8_t* done_env, int32_t n, int32_t agents_per_env, int64_t pos, void* stream) {
    if (int rc = push_check("replay_push", rp, s, s2, a, r_env, done_env, n, agents_per_env, pos)) return rc < 0 ? rc : 0;
    return push_launch("replay_push", rp, {s, s2, nullptr, a, r_env, done_env}, n, 1, agents_per_env, pos, stream);
}

int evx_replay_push_term(const evx_replay* rp, const evx_obs* s, const evx_obs* s2, const evx_obs* s2_term,
                         const int32_t* a, const double* r_env, const uint8_t* done_env, int32_t n,
                         int32_t agents_per_env, int64_t pos, void* stream) {
    if (int rc = push_check("replay_push_term", rp, s, s2, a, r_env, done_env, n, agents_per_env, pos))
        return rc < 0 ? rc : 0;
    return push_launch("replay_push_term", rp, {s, s2, s2_term, a, r_env, done_env}, n, 1, agents_per_env, pos, stream);
}

int evx_replay_push_blocks(const evx_replay* rp, const evx_obs* s, const evx_obs* s2, const evx_obs* s2_term,
                           const int32_t* a, const double* r_env, const uint8_t* done_env, int32_t n, int32_t nets,
                           int32_t agents_per_env, int64_t pos, void* stream) {
    if (!rp || !s || !s2 || !a || !r_env || !done_env) return fail(-22, "replay_push_blocks: NULL argument");
    if (int rc = ring_arrays_ok("replay_push_blocks", rp)) return rc;
    if (nets < 1 || nets > 64) return fail(-22, "replay_push_blocks: nets must be 1..64");
    if (n < 0 || (n & 1)) return fail(-22, "replay_push_blocks: rows per ring must be even and >= 0");
    if (rp->capacity < 1 || rp->capacity < n) return fail(-22, "replay_push_blocks: the capacity does not hold n rows");
    if (agents_per_env < 1 || n % agents_per_env)
        return fail(-22, "replay_push_blocks: rows per ring must be a multiple of agents_per_env");
    if (pos < 0 || pos >= rp->capacity) return fail(-22, "replay_push_blocks: pos outside [0, capacity)");
    if (n == 0) return 0;
    return push_launch("replay_push_blocks", rp, {s, s2, s2_term, a, r_env, done_env}, n, nets, agents_per_env, pos,
                       stream);
}

int evx_replay_sample(const evx_replay* rp, int64_t size, int32_t B, uint64_t seed, uint64_t offset, evx_obs* s,
                      evx_obs* s2, int32_t* a, float* r, uint8_t* done, int64_t* idx_out, void* stream) {
    if (!rp || size <= 0) return fail(-22, "replay: empty");
    if (B <= 0) return 0;
    if (size > rp->capacity) return fail(-22, "replay: size > capacity");
    if (B > size) return fail(-22, "replay: sample larger than population (random.sample)");
    if (int rc = ring_arrays_ok("replay_sample", rp)) return rc;
    if (!s || !s2 || !a || !r || !done) return fail(-22, "replay_sample: NULL argument");
    return sample_launch<WINDOW>("replay_sample", rp, {0, size, B, 1, 0, seed, offset}, s, s2, a, r, done, idx_out,
                                 stream);
}

int evx_replay_sample_window(const evx_replay* rp, int64_t base, int64_t count, int32_t B, uint64_t seed,
                             uint64_t offset, evx_obs* s, evx_obs* s2, int32_t* a, float* r, uint8_t* done,
                             int64_t* idx_out, void* stream) {
    if (!rp || count <= 0) return fail(-22, "replay: empty window");
    if (count > rp->capacity || base < 0 || base >= rp->capacity) return fail(-22, "replay: bad window");
    if (B <= 0) return 0;
    if (B > count) return fail(-22, "replay: sample larger than the window (random.sample)");
    if (int rc = ring_arrays_ok("replay_sample_window", rp)) return rc;
    if (!s || !s2 || !a || !r || !done) return fail(-22, "replay_sample_window: NULL argument");
    return sample_launch<WINDOW>("replay_sample_window", rp, {base, count, B, 1, 0, seed, offset}, s, s2, a, r, done,
                                 idx_out, stream);
}

int evx_replay_sample_agents(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                             uint64_t offset, evx_obs* s, evx_obs* s2, int32_t* a, float* r, uint8_t* done,
                             void* stream) {
    return sample_agents("replay_sample_agents", 0, rp, size, B, nets, seed, offset, s, s2, a, r, done, stream);
}

int evx_replay_sample_joint(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                            uint64_t offset, evx_obs* s, evx_obs* s2, int32_t* a, float* r, uint8_t* done,
                            void* stream) {
    return sample_agents("replay_sample_joint", 1, rp, size, B, nets, seed, offset, s, s2, a, r, done, stream);
}

int evx_replay_sample_blocks(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                             uint64_t offset, evx_obs* s, evx_obs* s2, int32_t* a, float* r, uint8_t* done,
                             void* stream) {
    if (!rp || !s || !s2 || !a || !r || !done) return fail(-22, "replay_sample_blocks: NULL argument");
    if (int rc = blocks_check("replay_sample_blocks", rp, size, B, nets)) return rc;
    if (B == 0) return 0;
    return sample_launch<BLOCKS>("replay_sample_blocks", rp, {0, size, B, nets, 0, seed, offset}, s, s2, a, r, done,
                                 nullptr, stream);
}

int evx_replay_nstep(const evx_replay* rp, const int64_t* idx, int32_t B, int64_t base, int64_t count, int64_t stride,
                     int32_t n_step, float gamma, evx_obs* s2, float* r, uint8_t* done, float* gamma_row, int32_t* len,
                     void* stream) {
    if (!rp || rp->capacity <= 0) return fail(-22, "replay_nstep: bad ring");
    if (!idx || !s2 || !r || !done || !gamma_row) return fail(-22, "replay_nstep: NULL argument");
    if (int rc = chain_ok("replay_nstep", rp, base, count, &stride, n_step, gamma)) return rc;
    if (B <= 0) return 0;
    if (!rp->s2 || !rp->r || !rp->done) return fail(-22, "replay_nstep: ring without s2 / r / done");
    hipLaunchKernelGGL(evxq::replay_nstep_kernel, dim3(nblk(B)), dim3(256), 0, (hipStream_t)stream, *rp, idx, (int)B,
                       base, count, stride, (int)n_step, gamma, s2, r, done, gamma_row, len);
    return hip_status("replay_nstep");
}

int evx_replay_sample_nstep_agents(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, int32_t joint,
                                   uint64_t seed, uint64_t offset, int64_t base, int64_t count, int64_t stride,
                                   int32_t n_step, float gamma, evx_obs* s, evx_obs* s2, int32_t* a, float* r,
                                   uint8_t* done, float* gamma_row, int32_t* len, int64_t* idx_out, void* stream) {
    const char* who = "replay_sample_nstep_agents";
    if (!rp || !s || !s2 || !a || !r || !done || !gamma_row) return failf(-22, "%s: NULL argument", who);
    if (rp->capacity <= 0) return failf(-22, "%s: bad ring", who);
    if (int rc = chain_ok(who, rp, base, count, &stride, n_step, gamma)) return rc;
    if (B <= 0) return 0;
    if (int rc = agents_ok(who, rp, size, B, nets, joint != 0)) return rc;
    if (int rc = ring_arrays_ok(who, rp)) return rc;
    hipLaunchKernelGGL((evxq::replay_sample_nstep_kernel<AGENTS, 1>), dim3(nblk(B), nets), dim3(256), 0,
                       (hipStream_t)stream, *rp, draw_args{0, size, B, nets, joint ? 1 : 0, seed, offset}, base, count, stride,
                       evxq::Nstep<1>{{n_step}, {gamma}}, s, s2, a, r, done, gamma_row, len, idx_out);
    return hip_status(who);
}

int evx_replay_sample_nstep_blocks(const evx_replay* rp, int64_t size, int32_t B, int32_t nets, uint64_t seed,
                                   uint64_t offset, int64_t base, int64_t count, int64_t stride,
                                   const int32_t* n_step, const float* gamma, evx_obs* s, evx_obs* s2, int32_t* a,
                                   float* r, uint8_t* done, float* gamma_row, int32_t* len, int64_t* idx_out,
                                   void* stream) {
    const char* who = "replay_sample_nstep_blocks";
    if (!rp || !n_step || !gamma || !s || !s2 || !a || !r || !done || !gamma_row)
        return failf(-22, "%s: NULL argument", who);
    if (int rc = blocks_check(who, rp, size, B, nets)) return rc;
    if (int rc = chain_blocks_ok(who, rp, base, count, &stride, n_step, gamma, nets)) return rc;
    if (B == 0) return 0;
    evxq::Nstep<64> nn{};
    std::copy(n_step, n_step + nets, nn.n);
    std::copy(gamma, gamma + nets, nn.gamma);
    hipLaunchKernelGGL((evxq::replay_sample_nstep_kernel<BLOCKS, 64>), dim3(nblk(B), (unsigned)nets), dim3(256), 0,
                       (hipStream_t)stream, *rp, draw_args{0, size, B, nets, 0, seed, offset}, base, count, stride, nn,
                       s, s2, a, r, done, gamma_row, len, idx_out);
    return hip_status(who);
}

int evx_gather_obs(const evx_obs* src, const int64_t* idx, int32_t n, evx_obs* dst, void* stream) {
    if (n <= 0) return 0;
    if (!src || !idx || !dst) return fail(-22, "gather_obs: NULL argument");
    hipLaunchKernelGGL(evxq::gather_rows_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, src, idx, n, dst);
    return hip_status("gather_obs");
}

}  // extern "C"
